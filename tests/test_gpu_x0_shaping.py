"""GPU: per-image x0 shaping - the statistics kernel (its order statistic bit for bit against torch.sort and the stated fp32 interpolation, its
variances and factor against fp64 inside the budgets of tests/test_x0_shaping_cpu.py), the eight shaped step forms against fp64 inside theirs,
mi355_ddpm_shaped_sample with shaping off (the six existing loops, bit for bit) and on (against the generic host loop, against the fp64
restatement tests/x0_shaping_ref.py driven by the same fp32 network, and away from the unshaped sampler), and the public path.

Tolerances: fused against the fp64 restatement rtol 2e-3 / atol 1e-3 (tests/test_gpu_unet.py SAMPLER_TOL); fused against generic 1e-4 (1 + 2|w|),
1e-4 unguided (tests/test_gpu_cfg.py); "away from the unshaped sampler": 5 x (atol + rtol max|x|) of SAMPLER_TOL.  The op tests use the CPU-derived
budgets only.  Tiny fp32 nets at 16x16 (tests/test_gpu_unet.py _tiny), B = 3, DDPM(100) on 7 steps even in logSNR.
"""
import math

import numpy as np
import pytest
import torch

from mi355.synth import randn
from tests import x0_shaping_ref as XR
from tests.test_gpu_ddpm_respace import _banded, _bits, _report, _unband
from tests.test_x0_shaping_cpu import (factor_budget, rows_for, shaped_budget, sigma_budget, step_cases, step_operands)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STOL = dict(rtol=2e-3, atol=1e-3)
B, S = 3, 16
W = 4.0
SHAPING = (0.9, None, 0.7)
_CACHE = {}


def _same_bits(got, want):
    """Bit equality of two fp32 tensors, a NaN matching any NaN."""
    g, w = got.cpu(), want.cpu()
    nan = torch.isnan(w)
    return bool(torch.equal(torch.isnan(g), nan)) and bool(torch.equal(_bits(g)[~nan], _bits(w)[~nan]))


def _quantiles(per):
    return sorted({min(1.0, 1.0 / per), min(1.0, 2.5 / per), 0.5, 0.995, 1.0})


def _stats(x, eps, cr, crm1, shaping, w=None):
    from mi355.ops import default_ops as ops

    shape, det = ops.x0_shape_stats(x, eps, cr, crm1, shaping, w=w, detail=True)
    torch.cuda.synchronize()
    return shape.cpu(), det.cpu()


# ---- 1. the selection is exact -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", [1, 2, 5, 63, 64, 65, 255, 257, 3 * 8 * 8, 3 * 32 * 32 + 3, 3 * 128 * 128])
def test_selection_is_exact_on_random_images(per):
    """s_raw is, bit for bit, lo + frac (hi - lo) of the sorted fp32 |x0|, x0 formed in eager fp32; three different images per call, the state one
    float off the 16-byte grid."""
    cr, crm1 = 1.8, 1.5
    xb, x = _banded(randn(9100 + per % 1000, B, per) * torch.tensor([[0.6], [1.0], [2.0]]), 1)
    eps = (randn(9200 + per % 1000, B, per) * 0.7).to(DEV)
    x0 = (cr * x - crm1 * eps).cpu()
    for p in _quantiles(per):
        for s_max in (None, 1.25):
            shape, det = _stats(x, eps, cr, crm1, (p, s_max, 0.0))
            want_s, want_raw = XR.threshold(x0, p, s_max)
            assert want_raw.dtype == torch.float32
            assert _same_bits(det[:, 2], want_raw), (per, p, det[:, 2], want_raw)
            assert _same_bits(shape[:, 1], want_s) and torch.equal(shape[:, 0], torch.ones(B)), (per, p)
    _unband(xb, B * per, 1)
    assert len({float(v) for v in want_raw}) == B or per == 1     # the images differ: a cross-image mix-up would show


def _adversarial(per, k, rng):
    """Images [per] of exact fp32 values planted as x (c_recip = 1, c_recipm1 = 0: x0 = x), signs and order shuffled."""
    u32 = lambda a: np.asarray(a, np.uint32).view(np.float32)   # noqa: E731
    k1 = min(k + 1, per - 1)
    out = {}
    out["all_equal"] = np.full(per, 1.37, np.float32)
    v = np.full(per, 2.5, np.float32)
    v[:k + 1] = 0.75
    out["two_values_split_at_k"] = v                                     # the k-th is 0.75, the next one 2.5
    v = np.sort(rng.uniform(0.1, 3.0, per).astype(np.float32))
    v[max(k - 1, 0):min(k1 + 2, per)] = v[k]
    out["ties_straddling_k"] = v
    v = rng.uniform(0.5, 2.0, per).astype(np.float32)
    v[:max(k1 + 1, per // 2)] = 0.0
    v[:per // 3] = -0.0
    out["signed_zeros"] = v
    out["denormals"] = u32(rng.integers(1, 1 << 20, per))
    out["lowest_byte_only"] = u32(0x3FC00000 + rng.integers(0, 256, per))
    out["top_byte_only"] = u32((rng.integers(0, 0x7F, per).astype(np.uint32) << 24) | np.uint32(0x00123456))
    v = rng.uniform(0.1, 3.0, per).astype(np.float32)
    v[per // 2] = np.inf
    out["one_inf"] = v
    v = rng.uniform(0.1, 3.0, per).astype(np.float32)
    v[per // 3] = np.nan
    out["one_nan"] = v
    order = ["all_equal", "two_values_split_at_k", "one_inf", "ties_straddling_k", "signed_zeros", "denormals", "lowest_byte_only", "top_byte_only",
             "one_nan"]           # groups of three: the infinity (whose interpolation can be inf - inf) not beside the NaN image
    out = {n: out[n] for n in order}
    for name, v in out.items():
        if per > 1:
            v *= np.where(rng.random(per) < 0.5, np.float32(-1), np.float32(1))
            rng.shuffle(v)
    return out


@pytest.mark.parametrize("per", [5, 65, 257, 3 * 32 * 32 + 3])
def test_selection_is_exact_on_adversarial_images(per):
    rng = np.random.default_rng(9300 + per)
    worst = []
    for p in _quantiles(per):
        k, _ = XR.position(p, per)
        imgs = _adversarial(per, k, rng)
        names = list(imgs)
        for g in range(0, len(names), B):
            grp = names[g:g + B]
            x = torch.from_numpy(np.stack([imgs[n] for n in grp])).to(DEV)
            eps = torch.from_numpy(rng.standard_normal((B, per)).astype(np.float32)).to(DEV)
            shape, det = _stats(x, eps, 1.0, 0.0, (p, None, 0.0))
            x0 = (1.0 * x - 0.0 * eps).cpu()
            assert _same_bits(x0.abs(), x.abs().cpu())
            want_s, want_raw = XR.threshold(x0, p)
            assert _same_bits(det[:, 2], want_raw), (per, p, grp, det[:, 2], want_raw)
            assert _same_bits(shape[:, 1], want_s), (per, p, grp)
            for j, n in enumerate(grp):
                if n == "one_nan":    # that image only
                    assert math.isnan(float(shape[j, 1])) and not torch.isnan(shape[torch.arange(B) != j, 1]).any()
                    worst.append(n)
    assert worst


# ---- 2. the variances and the factor -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", [1, 5, 257, 3 * 32 * 32 + 3])
def test_sigmas_and_factor_vs_fp64(per):
    """Guided, per-image w_dev, per % 4 != 0 (groups of four straddle images), image 2 constant (sigma_g == 0, f = 1)."""
    phi = 0.7
    ec = randn(9400 + per % 1000, B, per) * 1.3 + 0.4
    eu = randn(9500 + per % 1000, B, per)
    ec[2], eu[2] = 0.75, 0.75
    w = torch.tensor([4.0, 0.5, 2.0])
    x = randn(9600 + per % 1000, B, per).to(DEV)
    e2 = torch.cat((ec, eu)).to(DEV)
    eg = (e2[B:] + (e2[:B] - e2[B:]) * w.to(DEV)[:, None]).cpu()    # u + w (c - u) in eager fp32: the kernel's cfg_mix, bit for bit
    shape, det = _stats(x, e2, 1.8, 1.5, (0.9, None, phi), w=w.to(DEV))
    sc, bc = sigma_budget(ec.numpy())
    sg, bg = sigma_budget(eg.numpy())
    f, bf = factor_budget(sc, bc, sg, bg, phi)
    rc, rg = np.abs(det[:, 0].double().numpy() - sc) / np.maximum(bc, 1e-300), np.abs(det[:, 1].double().numpy() - sg) / np.maximum(bg, 1e-300)
    rf = np.abs(shape[:, 0].double().numpy() - f) / bf
    print(f"per = {per}: err / budget sigma_c {rc.max():.3f}, sigma_g {rg.max():.3f}, f {rf.max():.3f}")
    assert (np.abs(det[:, 0].double().numpy() - sc) <= bc).all() and (np.abs(det[:, 1].double().numpy() - sg) <= bg).all()
    assert float(det[2, 1]) == 0.0 and float(shape[2, 0]) == 1.0 and (rf <= 1.0).all()
    # the threshold is taken on the rescaled eps: s_raw from the kernel's own f, bit for bit
    x0 = (1.8 * x - 1.5 * (shape[:, 0].to(DEV)[:, None] * eg.to(DEV))).cpu()
    assert _same_bits(det[:, 2], XR.threshold(x0, 0.9)[1])
    # phi = 0: f = 1 and the sigmas are still reported; unguided: both are the eps's
    s0, d0 = _stats(x, e2, 1.8, 1.5, (0.9, None, 0.0), w=w.to(DEV))
    assert torch.equal(s0[:, 0], torch.ones(B)) and torch.equal(d0[:, :2], det[:, :2])
    s1, d1 = _stats(x, e2[:B].contiguous(), 1.8, 1.5, (0.9, None, 0.0))
    assert torch.equal(d1[:, 0], d1[:, 1]) and torch.equal(d1[:, 0], det[:, 0])


# ---- 3. the shaped steps against fp64 --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,per,off", [(105, 35, 0), (105, 35, 1), (768, 256, 1)])
@pytest.mark.parametrize("philox", [False, True])
def test_shaped_step_ops_vs_fp64(n, per, off, philox):
    """All eight forms on NaN-banded buffers: inside the CPU-derived budgets, rows (1, 1) bit-identical to the unshaped op, guard bands untouched."""
    from mi355.ops import default_ops as ops

    worst = {}
    Bn = n // per
    unshaped = {"ddpm": lambda x, e, z, ph, a, b, c, h: ops.ddpm_step_(x, e, z, a, b, c[0], c[1], c[2], ph),
                "ddim": lambda x, e, z, ph, a, b, c, h: ops.ddim_step_(x, e, a, b, c[0]),
                "ddim_eta": lambda x, e, z, ph, a, b, c, h: ops.ddim_eta_step_(x, e, z, a, b, c[0], c[1], ph),
                "dpmpp": lambda x, e, z, ph, a, b, c, h: ops.dpmpp_step_(x, e, h, a, b, *c)}
    for j, (kind, a, b, c) in enumerate(step_cases()):
        x, eps, z, hist = step_operands(kind, n, a, b, 100 * j + n)
        f, s = rows_for(n, per, 9 * j + n)
        ph = None
        if z is not None and philox:
            ph = (1234 + j, 4 * j)
            z = ops.randn((n,), DEV, *ph).cpu().numpy()
        eu = randn(9700 + j, n).numpy()
        w = torch.tensor([1.75, 0.5, 3.0][:Bn])
        for guided in (False, True):
            if guided:
                e2 = torch.cat((torch.from_numpy(eps), torch.from_numpy(eu))).to(DEV).view(2, Bn, per)
                e_in = (e2[1] + (e2[0] - e2[1]) * w.to(DEV)[:, None]).cpu().numpy().reshape(-1)
            else:
                e_in = eps
            with np.errstate(invalid="ignore"):
                want, x0, bound, bound0 = shaped_budget(kind, x, e_in, f, s, per, a, b, c, z, hist)
            res = {}
            for rows in ("rows", "ones", "none"):
                fs = np.stack((f, s), 1) if rows == "rows" else np.ones((Bn, 2), np.float32)
                shape = None if rows == "none" else torch.from_numpy(fs).to(DEV)
                tx = torch.from_numpy(x)
                bx, vx = _banded(torch.cat((tx, tx + 3.0)) if guided else tx, off)
                be, ve = _banded(torch.cat((torch.from_numpy(eps), torch.from_numpy(eu))) if guided else torch.from_numpy(eps), off)
                bh, vh = _banded(torch.from_numpy(hist), off) if hist is not None else (None, None)
                zt = torch.from_numpy(z).to(DEV).view(Bn, per) if (z is not None and ph is None) else None
                lead = (2 * Bn, per) if guided else (Bn, per)
                kw = dict(sigma=c[-1] if kind in ("ddpm", "ddim_eta") else 0.0, z=zt, philox=ph if zt is None else None,
                          hist=vh.view(Bn, per) if vh is not None else None, w=w.to(DEV) if guided else None)
                abc = dict(ddpm=(c[0], c[1]), ddim=(c[0],), ddim_eta=(c[0],), dpmpp=c)[kind]
                ops.x0_shaped_step_(kind, vx.view(lead), ve.view(lead), shape, a, b, *abc, **kw)
                torch.cuda.synchronize()
                both = _unband(bx, vx.numel(), off)
                if guided:
                    assert torch.equal(_bits(both[:n]), _bits(both[n:])), "the two halves differ"
                res[rows] = (both[:n].clone(), _unband(bh, n, off).clone() if bh is not None else None)
            assert torch.equal(_bits(res["ones"][0]), _bits(res["none"][0])), (kind, guided)
            if hist is not None:
                assert torch.equal(_bits(res["ones"][1]), _bits(res["none"][1]))
            if not guided:   # and the unshaped op of old gives those bits too
                bx, vx = _banded(torch.from_numpy(x), off)
                bh, vh = _banded(torch.from_numpy(hist), off) if hist is not None else (None, None)
                zt = torch.from_numpy(z).to(DEV) if (z is not None and ph is None) else None
                unshaped[kind](vx, torch.from_numpy(eps).to(DEV), zt, ph if zt is None else None, a, b, c, vh)
                torch.cuda.synchronize()
                assert torch.equal(_bits(_unband(bx, n, off)), _bits(res["none"][0])), kind
            got = res["rows"][0].double().numpy()
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and nan.sum() == 1
            key = kind + ("_cfg" if guided else "")
            worst[key] = max(worst.get(key, 0.0), float((np.abs(got - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max()))
            if hist is not None:    # the history keeps the shaped D
                gd = res["rows"][1].double().numpy()
                assert (np.abs(gd - x0)[~nan] <= bound0[~nan]).all()
            assert not torch.equal(_bits(res["rows"][0]), _bits(res["ones"][0]))
    print(f"n = {n}, per = {per}, off = {off}, philox = {philox}: max err / budget {({k: round(v, 3) for k, v in worst.items()})}")
    assert len(worst) == 8 and max(worst.values()) <= 1.0, worst


# ---- nets, inputs ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets():
    from tests.test_gpu_unet import _tiny

    return {1: _tiny(1, 1, 1001, "fp32"), 2: _tiny(2, 1, 1002, "fp32")}   # in_channels -> (cfg, net, sd)


def _inputs():
    xT = randn(8601, B, 1, S, S)
    cond = (randn(8602, B, 1, S, S) * 0.5).clamp(-1, 1)
    cond[:, :, 4:10, 5:11] = -2.0
    return xT, cond


def _chain():
    from image_diffusion.sde_diffusion import DDPM

    if "chain" not in _CACHE:
        d = DDPM(100)
        _CACHE["chain"] = d.respace(d.logsnr_steps(7))
    return _CACHE["chain"]


def _draws(n=40):
    return randn(8700, n, B, 1, S, S)


# ---- 4. off means off --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loop", ["prior", "amortized_corrector", "repaint", "guided_ddim_eta", "dpm", "dpm_guided"])
@pytest.mark.parametrize("off", [None, (0.0, 0.0, 0.0), (0.0, 2.0, 0.0)])
def test_shaping_off_is_the_existing_entry_point(nets, loop, off):
    from image_diffusion.conditioning import repaint_walk
    from mi355 import _lib

    r = _chain()
    T = r.host_tables()
    xT, cond = (t.to(DEV) for t in _inputs())
    noise = _draws().to(DEV)
    sched = dict(timesteps=r.timesteps, train_steps=r.base_Ns)
    coefs = r.dpm_solver_coefs(2)
    cin, kw = {"prior": (1, dict(mode=_lib.DDPM_PRIOR, noise=noise)),
               "amortized_corrector": (2, dict(mode=_lib.DDPM_AMORTIZED, cond=cond, noise=noise, n_corrector=1)),
               "repaint": (1, dict(mode=_lib.DDPM_REPLACEMENT, cond=cond, noise=noise, start_fraction=0.8, walk=repaint_walk(r.Ns, 2, 2), **sched)),
               "guided_ddim_eta": (2, dict(mode=_lib.DDIM, cond=cond, noise=noise, guidance_scale=W, ddim_sigma=r.ddim_sigma(0.5), **sched)),
               "dpm": (1, dict(**sched)), "dpm_guided": (2, dict(cond=cond, guidance_scale=W, **sched))}[loop]
    eng = nets[cin][1].engine(DEV)
    if loop.startswith("dpm"):
        want = eng.ddpm_multistep(xT.clone(), T, coefs, **kw)
        got = eng.ddpm_shaped(xT.clone(), T, off, mode=_lib.DDIM, coefs=coefs, **kw)
    else:
        want = eng.ddpm_sample(xT.clone(), T, **kw)
        got = eng.ddpm_shaped(xT.clone(), T, off, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)) and (want - xT).abs().max() > 1e-2
    eng.check()


# ---- 5. on means on, and right -------------------------------------------------------------------------------------------------------------------------

def _net_eps(nets, cin, ddpm):
    """eps(net_in, k) from the fp32 HIP network itself: the restatement's arithmetic is fp64, its network outputs the sampler's own."""
    net = nets[cin][1]

    def eps(net_in, k):
        t = torch.full((net_in.shape[0],), ddpm.time(k), dtype=torch.float32, device=DEV)
        return net(net_in.float().to(DEV).contiguous(), t).cpu()

    return eps


@pytest.mark.parametrize("case", ["guided_ddim", "guided_ancestral", "plain_ddim", "guided_dpm", "guided_ddim_per_image_w"])
def test_shaped_samplers(nets, case):
    from image_diffusion import sampling
    from image_diffusion.conditioning import ClassifierFreeGuidance
    from image_diffusion.likelihoods import InPainting

    base = _chain()
    guided = case != "plain_ddim"
    shaping = SHAPING if guided else (0.9, None, 0.0)
    r = base.with_x0_shaping(dynamic_threshold=shaping[0], guidance_rescale=shaping[2])
    assert r.x0_shaping is not None and r.timesteps == base.timesteps
    lik = InPainting(patch_size=6, pad_value=-2)
    xT, cond = _inputs()
    xT = 1.5 * xT                                    # x0_hat beyond [-1, 1] on a good share of the pixels: asserted below
    noise = _draws()
    cin = 2 if guided else 1
    w = torch.tensor([4.0, 2.5, 5.5]) if case.endswith("per_image_w") else (W if guided else None)
    wd = w.to(DEV) if isinstance(w, torch.Tensor) else w
    net = nets[cin][1]

    def make(eps_model, ddpm):
        if case == "guided_ancestral":
            return sampling.get_conditional_sample_fn(eps_model, ddpm, ClassifierFreeGuidance(1.0, 0, 0.1, W), lik)
        if case == "guided_dpm":
            return sampling.get_dpm_solver_sample_fn(eps_model, ddpm, lik, guidance_scale=wd, order=2)
        return sampling.get_ddim_sample_fn(eps_model, ddpm, lik, guidance_scale=wd)

    args = (xT.to(DEV), cond.to(DEV)) if guided else (xT.to(DEV),)
    fast = sampling.make_eps_model(net, r)
    generic = lambda xi, i: fast(xi, i)   # noqa: E731  (untagged: the host loop over the stats and step ops)
    with sampling.injected_noise(list(noise)):
        got = make(fast, r)(*args).cpu()
        gen = make(generic, r)(*args).cpu()
        plain = make(sampling.make_eps_model(net, base), base)(*args).cpu()
    kind = {"guided_ancestral": "ancestral", "guided_dpm": "dpmpp"}.get(case, "ddim")
    log = []
    ref, used, n_eval = XR.sample(_net_eps(nets, cin, r), r.host_tables(), xT, noise, kind=kind, shaping=shaping, cond=cond if guided else None,
                                  none_value=-2.0, w=w, coefs=r.dpm_solver_coefs(2) if kind == "dpmpp" else None, log=log)
    assert n_eval == r.Ns * (2 if guided else 1)
    smax = torch.stack([s for _, _, s in log]).max(dim=0).values
    fall = torch.stack([f for _, f, _ in log])
    print(f"{case}: max s per image {smax.tolist()}, f in [{float(fall.min()):.3f}, {float(fall.max()):.3f}]")
    assert bool((smax > 1.0).all()), "the thresholds never left 1: the test shows nothing"
    e1 = _report(f"{case}: fused vs fp64 restatement", got, ref)
    e2 = _report(f"{case}: fused vs generic", got, gen)
    e3 = _report(f"{case}: shaped vs unshaped", got, plain)
    assert float(got.abs().max()) <= 1.0 and bool(torch.isfinite(got).all())
    wmax = float(w.abs().max()) if isinstance(w, torch.Tensor) else (abs(w) if w is not None else 0.0)
    gb = 1e-4 * (1 + 2 * wmax) if guided else 1e-4
    torch.testing.assert_close(got, gen, rtol=gb, atol=gb)
    torch.testing.assert_close(got.double(), ref, **STOL)
    assert e3 >= 5 * (STOL["atol"] + STOL["rtol"] * float(plain.abs().max())), e3
    assert np.isfinite(e1) and np.isfinite(e2)
    net.engine(DEV).check()


# ---- 6. the public path ---------------------------------------------------------------------------------------------------------------------------------

def test_public_path_is_one_library_call(nets, monkeypatch):
    from image_diffusion import sampling
    from image_diffusion.conditioning import ClassifierFreeGuidance, ReconstructionGuidance
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib

    lik = InPainting(patch_size=6, pad_value=-2)
    xT, cond = (t.to(DEV) for t in _inputs())
    d = DDPM(25)
    net = nets[2][1]
    eng = net.engine(DEV)
    calls = []
    real = eng.ddpm_shaped
    monkeypatch.setattr(eng, "ddpm_shaped", lambda *a, **k: calls.append(k.get("mode")) or real(*a, **k))
    monkeypatch.setattr(eng, "ddpm_sample", lambda *a, **k: pytest.fail("the unshaped entry point ran"))
    monkeypatch.setattr(eng, "ddpm_multistep", lambda *a, **k: pytest.fail("the unshaped entry point ran"))
    # the launches of one guided evaluation: what the existing guided DDIM loop leaves behind
    type(eng).ddpm_sample(eng, xT.clone(), d.host_tables(), mode=_lib.DDIM, cond=cond, guidance_scale=W)
    n0 = eng.stats(B)["launches"]
    shaped = d.with_x0_shaping(dynamic_threshold=0.995)
    out = sampling.get_conditional_sample_fn(sampling.make_eps_model(net, shaped), shaped, ClassifierFreeGuidance(1.0, 0, 0.1, W), lik)(xT, cond)
    assert len(calls) == 1 and eng.stats(B)["launches"] == n0 + 2 and n0 > 0
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0
    r = d.respace(10).with_x0_shaping(dynamic_threshold=0.995, guidance_rescale=0.5)
    em = sampling.make_eps_model(net, r)
    for fn in (sampling.get_ddim_sample_fn(em, r, lik, guidance_scale=W), sampling.get_ddim_sample_fn(em, r, lik, guidance_scale=W, eta=0.5),
               sampling.get_dpm_solver_sample_fn(em, r, lik, guidance_scale=W)):
        calls.clear()
        out = fn(xT, cond)
        assert len(calls) == 1 and eng.stats(B)["launches"] == n0 + 2
        assert bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0 and (out - xT).abs().max() > 1e-2
    eng.check()
    with pytest.raises(NotImplementedError, match="with_x0_shaping"):
        sampling.get_conditional_sample_fn(sampling.make_eps_model(nets[1][1], shaped), shaped, ReconstructionGuidance(1.0, 1.0, "before", 0, 0.1), lik)
    with pytest.raises(ValueError, match="guided"):
        sampling.get_ddim_sample_fn(em, r, lik)(xT, cond)
