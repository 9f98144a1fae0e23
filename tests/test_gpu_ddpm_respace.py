"""GPU: DDPM sampling on a sub-sequence of the training steps - the three new step kernels against fp64 from their fp32 inputs (the
budgets proven on the CPU in tests/test_ddpm_respace_cpu.py), the scheduled loop against the unscheduled one (bit-identical where the
schedule is the identity), respaced / DDIM(eta) / RePaint / reconstruction-guided samplers against the fp64 restatement
(tests/ddpm_respace_ref.py) driving the CPU oracle U-Net, the fused loop against the generic host loop, the refusals and launch counts.

Tolerances: the project's DDPM-sampler bound rtol 2e-3 / atol 1e-3 against the restatement (tests/test_gpu_unet.py SAMPLER_TOL); fused
against generic 1e-4, 1e-4 (1 + 2|w|) when guided (tests/test_gpu_cfg.py).  Tiny nets at 16x16, B = 3, injected noise unless said otherwise.
Observed on an MI355X: DESIGN.md section 8.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mi355.synth import rand_uniform, randn
from oracle import unet_ref
from tests import ddpm_respace_ref as R
from tests.test_ddpm_respace_cpu import EPS32, STEPS7, coefficient_cases, ddim_eta_budget, renoise_budget, step_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STOL = dict(rtol=2e-3, atol=1e-3)
GUARD = 64
B, S = 3, 16


def _report(tag, got, ref):
    d = float((got.double() - ref.double()).abs().max())
    print(f"{tag}: max|diff| {d:.3e}")
    return d


def _banded(t, off):
    """A copy of t on the device as a view into a NaN-filled buffer, GUARD floats of band on both sides, `off` floats off the 16-byte grid."""
    buf = torch.full((t.numel() + 2 * GUARD + 4,), float("nan"), device=DEV)
    view = buf[GUARD + off:GUARD + off + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _bits(t):
    return t.contiguous().view(torch.int32)


def _unband(buf, n, off):
    b = buf.cpu()
    assert bool(torch.isnan(b[:GUARD + off]).all()) and bool(torch.isnan(b[GUARD + off + n:]).all()), "a guard band was written"
    return b[GUARD + off:GUARD + off + n]


# ---- 1. the step kernels against fp64 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,off", [(105, 0), (768, 0), (768, 1)])
def test_step_ops_vs_fp64(n, off):
    from mi355.ops import default_ops as ops

    worst = dict(ddim=0.0, renoise=0.0)
    for k, eta, a, b, prev, sigma, ra, rb in coefficient_cases():
        x, eps, z = step_inputs(n, a, b, 100 * k + n)
        tx, te, tz = (torch.from_numpy(v) for v in (x, eps, z))
        for noisy in (True, False):
            want, bound = ddim_eta_budget(x, eps, z if noisy else None, a, b, prev, sigma)
            runs = []
            for _ in range(2):
                (bx, vx), (_, ve), (_, vz) = _banded(tx, off), _banded(te, off), _banded(tz, off)
                assert vx.data_ptr() % 16 == 4 * off
                ops.ddim_eta_step_(vx, ve, vz if noisy else None, a, b, prev, sigma)
                torch.cuda.synchronize()
                runs.append(_unband(bx, n, off))
            assert torch.equal(_bits(runs[0]), _bits(runs[1])), "two runs differ"
            got = runs[0].double().numpy()
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and nan.sum() == 1
            worst["ddim"] = max(worst["ddim"], float((np.abs(got - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max()))
        want, bound = renoise_budget(x, z, ra, rb)
        (bx, vx), (_, vz) = _banded(tx, off), _banded(tz, off)
        ops.renoise_(vx, vz, ra, rb)
        torch.cuda.synchronize()
        got = _unband(bx, n, off).double().numpy()
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        worst["renoise"] = max(worst["renoise"], float((np.abs(got - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max()))
    print(f"n = {n}, off = {off}: max err / bound: ddim_eta_step {worst['ddim']:.3f} (r = 10), renoise_step {worst['renoise']:.3f} (r = 3)")
    assert worst["ddim"] <= 1.0 and worst["renoise"] <= 1.0


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("Bn,img", [(3, (1, 5, 7)), (4, (3, 8, 8))])
def test_step_ops_identities_bit_exact(Bn, img, per_image):
    """sigma = 0 without noise is mi355_ddim_step; the guided step is the plain one on a torch-computed u + w (c - u); injected mi355_randn
    draws at the documented offset are the Philox path; n = 0 does nothing."""
    from mi355._lib import MI355BackendError
    from mi355.ops import default_ops as ops

    x = randn(7301, Bn, *img).to(DEV)
    eps2 = randn(7302, 2 * Bn, *img).to(DEV)
    z = randn(7303, Bn, *img).to(DEV)
    co = (1.8, 1.5, 0.6)
    assert torch.equal(ops.ddim_eta_step_(x.clone(), eps2[:Bn].contiguous(), None, *co, 0.0), ops.ddim_step_(x.clone(), eps2[:Bn].contiguous(), *co))
    w = torch.tensor([0.5 + 0.75 * b for b in range(Bn)], device=DEV) if per_image else 1.75
    wv = w.reshape(-1, *([1] * len(img))) if per_image else w
    d = eps2[:Bn] - eps2[Bn:]
    eg = (eps2[Bn:] + d * wv).contiguous()
    n = x.numel()
    off = (n + 3) // 4 * 4 * 2        # draw 2 of a loop over this state
    for zz, ph in ((z, None), (None, (77, off)), (None, None)):
        exp = ops.ddim_eta_step_(x.clone(), eg, zz, *co, 0.3, philox=ph)
        x2 = torch.cat((x, x + 5.0))   # the second half is never read
        ops.ddim_eta_cfg_step_(x2, eps2, zz, w, *co, 0.3, philox=ph)
        assert torch.equal(x2[:Bn], exp) and torch.equal(x2[Bn:], exp), (zz is None, ph)
    zd = ops.randn(tuple(x.shape), DEV, 77, off)
    assert torch.equal(ops.ddim_eta_step_(x.clone(), eg, zd, *co, 0.3), ops.ddim_eta_step_(x.clone(), eg, None, *co, 0.3, philox=(77, off)))
    assert torch.equal(ops.renoise_(x.clone(), zd, 0.9, 0.4), ops.renoise_(x.clone(), None, 0.9, 0.4, philox=(77, off)))
    assert (ops.renoise_(x.clone(), zd, 0.9, 0.4) - x).abs().max() > 0.05
    with pytest.raises(MI355BackendError, match="multiple of 4"):
        ops.ddim_eta_step_(x.clone(), eg, None, *co, 0.3, philox=(77, 6))
    with pytest.raises(MI355BackendError, match="sigma"):
        ops.ddim_eta_step_(x.clone(), eg, None, *co, -0.3)
    e = torch.empty(0, *img, device=DEV)
    ops.ddim_eta_step_(e, e, None, *co, 0.3)
    ops.ddim_eta_cfg_step_(e, e, None, 2.0, *co, 0.3)
    ops.renoise_(e, None, 0.9, 0.4)
    torch.cuda.synchronize()


# ---- nets, inputs, the restatement's eps -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets():
    from tests.test_gpu_unet import _tiny

    return {1: _tiny(1, 1, 1001, "fp32"), 2: _tiny(2, 1, 1002, "fp32")}   # in_channels -> (cfg, net, sd)


def _inputs():
    xT = randn(7601, B, 1, S, S)
    cond = (randn(7602, B, 1, S, S) * 0.5).clamp(-1, 1)
    cond[:, :, 4:10, 5:11] = -2.0
    return xT, cond


def _draws(n, base=7700):
    return [randn(base + j, B, 1, S, S) for j in range(n)]


def _ref_eps(nets, cin, ddpm, fwd=unet_ref.unet_forward):
    cfg, _, sd = nets[cin]
    return lambda net_in, k: fwd(sd, cfg, net_in.float(), torch.full((net_in.shape[0],), ddpm.time(k), dtype=torch.float32))


def _schedules():
    from image_diffusion.sde_diffusion import DDPM

    return {"7of100": DDPM(100).respace(STEPS7), "25of1000": DDPM(1000).respace(25)}


# ---- 2. the loop changes nothing old ------------------------------------------------------------------------------------------------------

def test_identity_schedule_is_bit_identical_to_the_unscheduled_loop(nets):
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib

    Ns = 25
    ddpm = DDPM(Ns)
    T = ddpm.host_tables()
    xT, cond = (t.to(DEV) for t in _inputs())
    noise = torch.stack(_draws(3 * Ns)).to(DEV)
    ident = dict(timesteps=tuple(range(Ns)), train_steps=Ns)
    cases = [("prior", 1, dict(mode=_lib.DDPM_PRIOR)), ("amortized", 2, dict(mode=_lib.DDPM_AMORTIZED, cond=cond)),
             ("amortized_corr1", 2, dict(mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1)),
             ("replacement", 1, dict(mode=_lib.DDPM_REPLACEMENT, cond=cond, start_fraction=0.5, noise_condition=True)),
             ("replacement_corr1", 1, dict(mode=_lib.DDPM_REPLACEMENT, cond=cond, start_fraction=0.5, n_corrector=1)),
             ("ddim", 2, dict(mode=_lib.DDIM, cond=cond)),
             ("guided_amortized_corr1", 2, dict(mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1, guidance_scale=2.0)),
             ("guided_ddim", 2, dict(mode=_lib.DDIM, cond=cond, guidance_scale=2.0))]
    for name, cin, kw in cases:
        eng = nets[cin][1].engine(DEV)
        kw = dict(kw, delta=0.1, tmin=ddpm.tmin, tmax=ddpm.tmax)
        for nz in (dict(noise=noise), dict(seed=4242)):
            a = eng.ddpm_sample(xT.clone(), T, **kw, **nz)
            la = eng.stats(B)["launches"]
            b = eng.ddpm_sample(xT.clone(), T, **kw, **nz, **ident)
            lb = eng.stats(B)["launches"]
            assert torch.equal(_bits(a), _bits(b)), (name, list(nz))
            assert la == lb, (name, la, lb)
            assert (a - xT).abs().max() > 1e-2
        eng.check()


# ---- 3. respaced samplers against the restatement, fused against generic ------------------------------------------------------------------------

MODES = ["prior", "amortized", "amortized_corr1", "replacement", "ddim_eta0", "ddim_eta0.5", "ddim_eta1", "guided_ddim_eta0.5"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sched", ["7of100", "25of1000"])
def test_respaced_samplers_vs_restatement(nets, sched, mode):
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, Replacement
    from image_diffusion.likelihoods import InPainting

    r = _schedules()[sched]
    K = r.Ns
    T = {k: v.numpy() for k, v in r.host_tables().items()}
    lik = InPainting(patch_size=6, pad_value=-2)
    xT, cond = _inputs()
    draws = _draws(3 * K)
    cin = 1 if mode in ("prior", "replacement") else 2
    net = nets[cin][1]
    eps_ref = _ref_eps(nets, cin, r)
    fast = sampling.make_eps_model(net, r)
    generic = lambda xi, i: fast(xi, i)   # noqa: E731  (untagged: the host loop over the step ops)
    w = None
    if mode == "prior":
        ref, used, n_eval = R.sample(eps_ref, T, xT, draws, mode="prior")
        run = lambda e: sampling.get_prior_sample_fn(e, r, Replacement(0.1, 1.0, True, 0), lik)(xT.to(DEV))   # noqa: E731
    elif mode.startswith("amortized"):
        nc = int(mode.endswith("corr1"))
        ref, used, n_eval = R.sample(eps_ref, T, xT, draws, mode="amortized", cond=cond, amortized=True, n_corrector=nc, delta=0.1,
                                     tmin=r.tmin, tmax=r.tmax)
        run = lambda e: sampling.get_conditional_sample_fn(e, r, Amortized(0.9, nc, 0.1), lik)(xT.to(DEV), cond.to(DEV))   # noqa: E731
        assert n_eval == K * (1 + nc)
    elif mode == "replacement":
        ref, used, n_eval = R.sample(eps_ref, T, xT, draws, mode="replacement", cond=cond, start_fraction=0.5, noise_condition=True)
        run = lambda e: sampling.get_conditional_sample_fn(e, r, Replacement(0.1, 0.5, True, 0), lik)(xT.to(DEV), cond.to(DEV))   # noqa: E731
        assert used == int(K * 0.5) + K - 1
    else:
        eta = float(mode.split("eta")[1])
        w = 2.0 if mode.startswith("guided") else None
        sg = R.ddim_sigma64(T["alphas_cumprod"], T["alphas_cumprod_prev"], eta).astype(np.float32) if eta else None
        ref, used, n_eval = R.sample(eps_ref, T, xT, draws, mode="ddim", cond=cond, amortized=True, ddim_sigma=sg, w=w)
        run = lambda e: sampling.get_ddim_sample_fn(e, r, lik, guidance_scale=w, eta=eta)(xT.to(DEV), cond.to(DEV))   # noqa: E731
        assert used == (K - 1 if eta else 0)
    with sampling.injected_noise(draws):
        got = run(fast).cpu()
    with sampling.injected_noise(draws):
        gen = run(generic).cpu()
    # exactly the draws the restatement used: one fewer is refused by the fused loop
    if used:
        from mi355._lib import MI355BackendError

        with sampling.injected_noise(draws[:used - 1]), pytest.raises(MI355BackendError, match="injected noise exhausted"):
            run(fast)
        with sampling.injected_noise(draws[:used]):
            assert torch.equal(run(fast).cpu(), got)
    e1 = _report(f"{sched} {mode}: fused vs fp64 restatement", got, ref)
    e2 = _report(f"{sched} {mode}: fused vs generic", got, gen)
    assert (ref - xT.double()).abs().max() > 1e-2
    torch.testing.assert_close(got.double(), ref, **STOL)
    gb = 1e-4 * (1 + 2 * abs(w)) if w is not None else 1e-4
    torch.testing.assert_close(got, gen, rtol=gb, atol=gb)
    assert np.isfinite(e1) and np.isfinite(e2)


# ---- 4. RePaint ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noisy", [True, False])
def test_repaint(nets, noisy):
    from image_diffusion import sampling
    from image_diffusion.conditioning import RePaint, Replacement, repaint_walk
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM
    from mi355._lib import MI355BackendError

    r = DDPM(100).respace(6)
    K, sf = 6, 0.5
    T = {k: v.numpy() for k, v in r.host_tables().items()}
    lik = InPainting(patch_size=6, pad_value=-2)
    xT, cond = _inputs()
    walk = repaint_walk(K, 2, 2)
    downs = [a - 1 for a, b in zip(walk, walk[1:]) if b < a]
    ups = len(walk) - 1 - len(downs)
    # the header's count: pasting moves (noised) + downward moves not to level 0 + downward moves * n_corrector + upward moves
    want_draws = (sum(i < int(K * sf) for i in downs) if noisy else 0) + sum(i > 0 for i in downs) + ups
    assert len(downs) == 10 and ups == 4
    draws = _draws(want_draws + 3)
    net = nets[1][1]
    ref, used, n_eval = R.sample(_ref_eps(nets, 1, r), T, xT, draws, mode="replacement", cond=cond, start_fraction=sf, noise_condition=noisy,
                                 walk=R.repaint_levels(K, 2, 2))
    assert used == want_draws and n_eval == len(downs)
    fast = sampling.make_eps_model(net, r)
    asked = []
    generic = lambda xi, i: asked.append(int(i[0])) or fast(xi, i)   # noqa: E731
    rp = RePaint(0.1, sf, noisy, 0, 2, 2)
    with sampling.injected_noise(draws[:want_draws]):
        got = sampling.get_conditional_sample_fn(fast, r, rp, lik)(xT.to(DEV), cond.to(DEV)).cpu()
    with sampling.injected_noise(draws[:want_draws]):
        gen = sampling.get_conditional_sample_fn(generic, r, rp, lik)(xT.to(DEV), cond.to(DEV)).cpu()
    assert asked == downs   # one evaluation per downward move, at that move's step
    _report(f"repaint noisy={noisy}: fused vs fp64 restatement", got, ref)
    _report(f"repaint noisy={noisy}: fused vs generic", got, gen)
    torch.testing.assert_close(got.double(), ref, **STOL)
    torch.testing.assert_close(got, gen, rtol=1e-4, atol=1e-4)
    with sampling.injected_noise(draws[:want_draws - 1]), pytest.raises(MI355BackendError, match="injected noise exhausted"):
        sampling.get_conditional_sample_fn(fast, r, rp, lik)(xT.to(DEV), cond.to(DEV))
    # the resampling matters, and n_resample = 1 is Replacement itself
    outs = []
    for c in (RePaint(0.1, sf, noisy, 0, 2, 1), Replacement(0.1, sf, noisy, 0)):
        with sampling.injected_noise(draws):
            outs.append(sampling.get_conditional_sample_fn(fast, r, c, lik)(xT.to(DEV), cond.to(DEV)))
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and (outs[0].cpu() - got).abs().max() > 1e-2
    # device noise: the same walk from the Philox stream, reproducible under one seed
    torch.manual_seed(5)
    a = sampling.get_conditional_sample_fn(fast, r, rp, lik)(xT.to(DEV), cond.to(DEV))
    assert torch.isfinite(a).all() and a.abs().max() <= 1.0
    net.engine(DEV).check()


# ---- 5. ReconstructionGuidance on a respaced chain ------------------------------------------------------------------------------------------------

def test_reconstruction_guidance_on_a_respaced_chain(nets):
    from image_diffusion import sampling
    from image_diffusion.conditioning import ReconstructionGuidance
    from image_diffusion.likelihoods import LowResolution
    from image_diffusion.sde_diffusion import DDPM

    r = DDPM(100).respace(STEPS7)
    T = {k: v.numpy() for k, v in r.host_tables().items()}
    gamma, sf = 100.0, 0.5
    lik = LowResolution(4, 4)
    xT = randn(7801, B, 1, S, S)
    ylow = lik.sample(rand_uniform(7802, -1, 1, B, 1, S, S))
    draws = _draws(r.Ns, 7850)
    eps_ref = _ref_eps(nets, 1, r, unet_ref.unet_forward_diff)
    ref, used = R.recon_guidance_sample(eps_ref, T, xT, ylow, draws, gamma=gamma, start_fraction=sf)
    plain, _ = R.recon_guidance_sample(eps_ref, T, xT, ylow, draws, gamma=0.0, start_fraction=sf)
    assert used == r.Ns - 1
    with sampling.injected_noise(draws):
        got = sampling.get_conditional_sample_fn(sampling.make_eps_model(nets[1][1], r), r, ReconstructionGuidance(gamma, sf, "before", 0, 0.1), lik)(
            xT.to(DEV), ylow.to(DEV)).cpu()
    _report("respaced reconstruction guidance vs fp64 restatement", got, ref)
    print(f"   the guidance moved the result by max {float((ref - plain).abs().max()):.3e}")
    assert float((ref - plain).abs().max()) > 10 * STOL["atol"]
    torch.testing.assert_close(got.double(), ref, **STOL)
    # an eps_model built for another schedule is refused (it would be evaluated at the wrong times)
    with pytest.raises(NotImplementedError):
        sampling.get_conditional_sample_fn(sampling.make_eps_model(nets[1][1], DDPM(7)), r, ReconstructionGuidance(gamma, sf, "before", 0, 0.1), lik)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------

def test_schedule_refusals(nets):
    from mi355 import _lib

    L = _lib.lib()
    from image_diffusion.sde_diffusion import DDPM

    r = DDPM(100).respace(STEPS7)
    K = r.Ns
    T = r.host_tables()
    xT, cond = (t.to(DEV) for t in _inputs())
    x = xT.clone()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    ones = (C.c_float * K)(*([0.5] * K))
    down = list(range(K, -1, -1))

    def sched(steps=STEPS7, train=100, sigma=None, walk=None, ra=None, rb=None):
        sd = _lib.DDPMScheduleC()
        keep = [(C.c_int32 * len(steps))(*steps)]
        sd.steps, sd.train_steps = C.cast(keep[0], ip), train
        if sigma is not None:
            keep.append((C.c_float * K)(*sigma))
            sd.ddim_sigma = C.cast(keep[-1], fp)
        if walk is not None:
            keep.append((C.c_int32 * len(walk))(*walk))
            sd.walk, sd.n_walk = C.cast(keep[-1], ip), len(walk)
        if ra is not None:
            sd.renoise_a, sd.renoise_b = C.cast(ra, fp), C.cast(rb, fp)
        return sd, keep

    def call(eng, sd, mode, guided=False):
        tb, keep = eng._ddpm_tables(T)
        opt = _lib.DDPMOptionsC(mode, 0, 0.1, 1e-5, 1.0, 1.0, 1, -2.0, -2.0, 0, 0)
        xp, cp = C.c_void_p(x.data_ptr()), C.c_void_p(cond.data_ptr())
        sp = C.byref(sd[0]) if sd is not None else None
        if guided:
            ws, wsb = eng._workspace_sized("mi355_ddpm_cfg_workspace_bytes", B)
            return L.mi355_ddpm_cfg_sample_sched(eng.handle, xp, 1, cp, None, 0, 2.0, None, C.byref(tb), C.byref(opt), sp, None, 0, B, ws, wsb, None)
        ws, wsb = eng.workspace(B)
        return L.mi355_ddpm_sample_sched(eng.handle, xp, 1, cp if mode != _lib.DDPM_PRIOR else None, C.byref(tb), C.byref(opt), sp, None, 0, B, ws, wsb,
                                         None)

    e1, e2 = nets[1][1].engine(DEV), nets[2][1].engine(DEV)
    up = [K, K - 1, K, K - 1] + down[2:]
    bad = [(None, "sched"), (sched(steps=[0, 3, 3, 17, 40, 41, 99]), "steps"), (sched(steps=[0, 3, 4, 17, 40, 41, 100]), "steps"),
           (sched(steps=[-1, 3, 4, 17, 40, 41, 99]), "steps"), (sched(train=0), "train_steps"), (sched(sigma=[0.5] * K), "ddim_sigma"),
           (sched(walk=down[1:]), "walk must start"), (sched(walk=down[:-1]), "walk must end"), (sched(walk=[K, K - 2] + down[3:]), "walk must move"),
           (sched(walk=[K, K + 1, K] + down[1:]), "walk must move"), (sched(walk=up), "renoise_a")]
    for sd, msg in bad:
        assert call(e1, sd, _lib.DDPM_PRIOR) == -1, msg
        assert msg.encode() in L.mi355_last_error(), (msg, L.mi355_last_error())
    for sg in ([0.5] * 3 + [-0.1] + [0.5] * 3, [float("nan")] + [0.5] * 6, [float("inf")] + [0.5] * 6):
        assert call(e2, sched(sigma=sg), _lib.DDIM) == -1 and b"ddim_sigma" in L.mi355_last_error()
    assert call(e2, sched(walk=up, ra=ones, rb=ones), _lib.DDPM_AMORTIZED, guided=True) == -1 and b"upward" in L.mi355_last_error()
    assert call(e2, None, _lib.DDPM_AMORTIZED, guided=True) == -1 and b"sched" in L.mi355_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(xT))   # nothing was launched: the state is untouched, byte for byte
    # the same walk with the arrays is accepted by the unguided entry, and a plain descent by the guided one
    assert call(e1, sched(walk=up, ra=ones, rb=ones), _lib.DDPM_PRIOR) == 0
    assert call(e2, sched(walk=down), _lib.DDPM_AMORTIZED, guided=True) == 0
    torch.cuda.synchronize()
    assert not torch.equal(x, xT)
    e1.check()
    e2.check()


# ---- 7. launch counts -----------------------------------------------------------------------------------------------------------------------

def test_respaced_step_launch_counts(nets):
    """The launches of a respaced step's evaluation are those of mi355_ddpm_sample's for the same mode (table path: no fill launch)."""
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib

    base = DDPM(25)
    r = DDPM(100).respace(STEPS7)
    xT, cond = (t.to(DEV) for t in _inputs())
    for cin, kw in ((1, dict(mode=_lib.DDPM_PRIOR)), (2, dict(mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1)),
                    (1, dict(mode=_lib.DDPM_REPLACEMENT, cond=cond, start_fraction=0.5)), (2, dict(mode=_lib.DDIM, cond=cond))):
        eng = nets[cin][1].engine(DEV)
        eng.ddpm_sample(xT.clone(), base.host_tables(), seed=3, **kw)
        n0 = eng.stats(B)["launches"]
        sg = dict(ddim_sigma=r.ddim_sigma(0.5)) if kw["mode"] == _lib.DDIM else {}
        eng.ddpm_sample(xT.clone(), r.host_tables(), seed=3, timesteps=r.timesteps, train_steps=r.base_Ns, **sg, **kw)
        n1 = eng.stats(B)["launches"]
        print(f"mode {kw['mode']}: launches of the last evaluation {n0} unscheduled, {n1} respaced")
        assert n0 == n1 and n0 > 0
        eng.check()
