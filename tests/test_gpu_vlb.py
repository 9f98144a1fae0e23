"""GPU: the variational bound of a DDPM net (mi355_ddpm_vlb, mi355_vlb_terms, mi355_vlb_prior, mi355_q_sample; image_diffusion.bound,
image_diffusion.loss_functions, evaluation.evaluate(vlb_fn=)).
  1. the terms and prior kernels against fp64 inside the budget tests/test_vlb_cpu.py derives: sizes that are no multiple of 4 or of the block,
     misaligned views between NaN guard bands, both steps kinds, learned and fixed variance, both CDFs, clip on and off, injected and Philox
     noise; two runs give the same bits; a fixed-variance call never reads the variance channels;
  2. mi355_ddpm_vlb against the host loop of ops (bit for bit) and against the fp64 restatement driven by the same fp32 network: plain,
     amortized with and without a condition, class labels, a time_scale chain; learned against fixed variance;
  3. a 3-output net under both fixed variances;
  4. identities that need no reference (a net that writes zeros; the mse column against mse_per_sample);
  5. one library call per batch and its launch count;
  6. the refusals that need a handle;
  7. get_loss_function; evaluate's bpd column.
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from mi355.synth import randn
from tests import vlb_ref as VR
from tests.test_ddpm_respace_cpu import EPS32
from tests.test_gpu_ddpm_respace import _banded, _bits
from tests.test_gpu_learned_variance import _chain, _lv_net
from tests.test_learned_variance_cpu import PERS
from tests.test_vlb_cpu import MODES, prior_budget, vlb_budget, vlb_cases, vlb_operands

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STOL = dict(rtol=2e-3, atol=1e-3)      # SAMPLER_TOL: the fused samplers against an fp64 restatement (tests/test_gpu_ddpm_respace.py)
B, S = 3, 16
FIELDS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")


# ---- 1. the kernels against fp64 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("philox", [False, True])
def test_vlb_terms_and_prior_vs_fp64(per, philox):
    from mi355.ops import default_ops as ops

    n = B * per
    worst = {}
    for j, (k, sc) in enumerate(vlb_cases()):
        x0, xk, eps, v, z = vlb_operands(per, sc, 700 * j + per)
        ph = None
        if philox:
            ph = (8642 + j, 4 * (j + 1))
            z = ops.randn((n,), DEV, *ph).cpu().numpy().reshape(B, per)
        kwsc = {name: sc[name] for name in VR.SCALARS}
        for learned, cdf, clip in MODES:
            kw = dict(k_is_zero=k == 0, learned=learned, cdf=cdf, clip=clip)
            want, bound = vlb_budget(x0, xk, eps, v, z, sc, **kw)
            # fixed variance: NaN in the variance channels, which must not be read
            out = torch.stack((torch.from_numpy(eps), torch.from_numpy(v) if learned else torch.full((B, per), float("nan"))), 1)      # [B, 2, per]
            runs = []
            for _ in range(2):
                views = [_banded(torch.from_numpy(a).view(B, 1, per), off)[1] for a, off in ((x0, 1), (xk, 3))]
                _, vo = _banded(out, 2)
                zt = _banded(torch.from_numpy(z).view(B, 1, per), 1)[1] if ph is None else None
                assert views[0].data_ptr() % 16 == 4 and views[1].data_ptr() % 16 == 12
                dst = torch.full((B, 5, 3), float("nan"), device=DEV)
                ops.vlb_terms(views[0], views[1], vo, z=zt, philox=ph, k_is_zero=k == 0, learned=learned, cdf=cdf, clip_denoised=clip, dst=dst[:, 2], **kwsc)
                torch.cuda.synchronize()
                got = dst.cpu()
                assert bool(torch.isnan(got[:, [0, 1, 3, 4]]).all()), "vlb_terms wrote outside its three numbers"
                runs.append(got[:, 2].clone())
            assert torch.equal(_bits(runs[0]), _bits(runs[1])), "two runs differ"
            got = runs[0].double().numpy()
            assert np.isfinite(got).all(), (k, learned, cdf, clip, got)
            ratio = np.abs(got - want) / bound
            key = ("decoder_" + cdf if k == 0 else "kl") + ("_learned" if learned else "_fixed")
            worst[key] = max(worst.get(key, 0.0), float(ratio.max()))
    # the prior term, and the total of planted step terms
    x0 = vlb_operands(per, vlb_cases()[0][1], 31 + per)[0]
    terms = randn(7100 + per, B, 7, 3).abs() * 3.0
    for sa, sb in ((0.0123, 0.99992), (0.4, 0.9165)):
        want, bound = prior_budget(x0, sa, sb)
        res = []
        for _ in range(2):
            vx = _banded(torch.from_numpy(x0).view(B, 1, per), 1)[1]
            res.append(ops.vlb_prior(vx, sa, sb, terms.to(DEV)).cpu())
        assert torch.equal(_bits(res[0]), _bits(res[1])), "two runs differ"
        got = res[0].double().numpy()
        worst["prior"] = max(worst.get("prior", 0.0), float((np.abs(got[:, 0] - want) / bound).max()))
        total = (terms[:, :, 0].double().sum(1) + res[0][:, 0].double()).float()
        assert torch.equal(_bits(res[0][:, 1]), _bits(total)) or float((res[0][:, 1] - total).abs().max()) <= float(np.spacing(np.float32(total.abs().max())))
        only = ops.vlb_prior(_banded(torch.from_numpy(x0).view(B, 1, per), 1)[1], sa, sb).cpu()
        assert torch.equal(_bits(only[:, 0]), _bits(res[0][:, 0])) and bool((only[:, 1] == 0).all())
    print(f"per = {per}, philox = {philox}: vlb_terms / vlb_prior max err / budget {({k: round(t, 3) for k, t in sorted(worst.items())})}")
    assert len(worst) == 7 and max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("per", PERS)
def test_q_sample_is_the_rounded_noising(per):
    from mi355.ops import default_ops as ops

    n = B * per
    x0, _, _, _, z = vlb_operands(per, vlb_cases()[2][1], 55 + per)
    sa, sb = 0.8123, 0.5832
    bx, vx = _banded(torch.from_numpy(x0).view(B, 1, per), 1)
    zt = torch.from_numpy(z).to(DEV).view(B, 1, per)
    got = ops.q_sample(vx, sa, sb, z=zt)
    assert torch.equal(_bits(got.cpu().view(B, per)), _bits(torch.from_numpy(VR.q_sample32(x0, z, sa, sb))))
    assert torch.equal(_bits(vx.cpu()), _bits(torch.from_numpy(x0).view(B, 1, per))), "x0 was written"
    ab = torch.tensor([[sa, sb]] * B, device=DEV)
    assert torch.equal(_bits(got), _bits(ops.lincomb_per_sample(vx.contiguous(), ab[:, 0].contiguous(), zt, ab[:, 1].contiguous())))
    zp = ops.randn((n,), DEV, 77, 8).view(B, 1, per)
    assert torch.equal(_bits(ops.q_sample(vx, sa, sb, philox=(77, 8))), _bits(ops.q_sample(vx, sa, sb, z=zp)))


# ---- nets, inputs, the host loop ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets():
    from image_diffusion.unet import UNetModel, param_shapes
    from mi355.synth import synth_state_dict
    from tests.test_gpu_unet import _tiny

    lab = UNetModel(image_size=S, in_channels=1, model_channels=32, out_channels=2, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
                    num_heads=2, num_classes=4, precision="fp32")
    sd = synth_state_dict(param_shapes(lab), 1031)
    sd["out.2.weight"][1:] *= 3.0
    sd["out.2.bias"][1:] *= 3.0
    lab.load_state_dict(sd)
    zero = _tiny(1, 1, 1041, "fp32")
    zsd = {k: t.clone() for k, t in zero[2].items()}
    zsd["out.2.weight"].zero_()
    zsd["out.2.bias"].zero_()
    zero[1].load_state_dict(zsd)
    return {(1, 2): _lv_net(1, 1, 1011)[1], (2, 2): _lv_net(2, 1, 1012)[1], "labels": lab.to(DEV), (3, 3): _tiny(3, 3, 1021, "fp32")[1],
            (1, 1): _tiny(1, 1, 1001, "fp32")[1], (2, 1): _tiny(2, 1, 1002, "fp32")[1], "zero": zero[1].to(DEV)}


def _data(C=1):
    """x0: 8-bit pixels in [-1, 1] with the two edge values present; a condition with a pad_value patch; K + 1 draws."""
    pix = torch.randint(0, 256, (B, C, S, S), generator=torch.Generator().manual_seed(4242 + C))
    pix.view(-1)[0], pix.view(-1)[1] = 0, 255
    x0 = (pix.float() / 127.5 - 1.0).contiguous()
    cond = x0.clone()
    cond[:, :, 4:10, 5:11] = -2.0
    return x0, cond, randn(8700 + C, 8, B, C, S, S)


def _host_loop(net, r, logs, x0, noise, *, learned, cond=None, y=None, seed=None, cdf="exact", clip=True, none_value=-2.0):
    """The bound as a loop of ops on the host: q_sample, engine.forward, vlb_terms per step, vlb_prior -> (terms [B, K, 3], summary [B, 2])."""
    from mi355.ops import default_ops as ops

    eng = net.engine(DEV)
    T = r.host_tables()
    K = r.Ns
    n_al = (x0.numel() + 3) // 4 * 4
    if cond is None and eng.in_channels == 2 * x0.shape[1]:
        cond = torch.full_like(x0, none_value)
    terms = torch.empty(x0.shape[0], K, 3, device=DEV)
    for k in reversed(range(K)):
        z = noise[K - 1 - k] if noise is not None else None
        ph = None if noise is not None else (seed, (K - 1 - k) * n_al)
        xk = ops.q_sample(x0, float(T["sqrt_alphas_cumprod"][k]), float(T["sqrt_one_minus_alphas_cumprod"][k]), z=z, philox=ph)
        out = eng.forward(xk, r.time(k), cond=cond, y=y)
        sc = dict(c_recip=float(T["sqrt_recip_alphas_cumprod"][k]), c_recipm1=float(T["sqrt_recipm1_alphas_cumprod"][k]),
                  coef1=float(T["posterior_mean_coef1"][k]), coef2=float(T["posterior_mean_coef2"][k]), true_log=float(logs["true_log"][k]))
        if learned:
            sc.update(min_log=float(logs["min_log"][k]), max_log=float(logs["max_log"][k]))
        else:
            sc.update(model_log=float(logs["model_log"][k]))
        ops.vlb_terms(x0, xk, out, z=z, philox=ph, k_is_zero=k == 0, learned=learned, cdf=cdf, clip_denoised=clip, dst=terms[:, k], **sc)
    return terms, ops.vlb_prior(x0, float(T["sqrt_alphas_cumprod"][K - 1]), float(T["sqrt_one_minus_alphas_cumprod"][K - 1]), terms)


def _net_out(net, r, y=None):
    def out(net_in, k):
        t = torch.full((net_in.shape[0],), r.time(k), dtype=torch.float32, device=DEV)
        return net(net_in.float().to(DEV).contiguous(), t, y).cpu()

    return out


def _as_dict(res):
    return {f: getattr(res, f).cpu() for f in FIELDS}


def _close(tag, got, ref):
    worst = 0.0
    for f in FIELDS:
        g, w = got[f].double(), torch.from_numpy(np.asarray(ref[f])).double()
        assert bool(torch.isfinite(g).all()), (tag, f)
        worst = max(worst, float(((g - w).abs() / (STOL["atol"] + STOL["rtol"] * w.abs())).max()))
        torch.testing.assert_close(g, w, **STOL, msg=lambda m, f=f: f"{tag}: {f}: {m}")
    print(f"{tag}: fused vs fp64 restatement, worst |diff| / (atol + rtol |ref|) = {worst:.3e}")


# ---- 2. the fused loop ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["plain", "amortized", "amortized_none", "labels", "time_scale", "plain_philox_tanh_unclipped"])
def test_fused_loop_vs_host_loop_and_fp64(nets, case):
    from image_diffusion import bound, sampling
    from image_diffusion.conditioning import Amortized
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM, cosine_betas
    from mi355.ops import default_ops as ops

    lik = InPainting(patch_size=6, pad_value=-2)
    r = _chain().with_learned_variance()
    if case == "time_scale":
        r = DDPM.from_betas(cosine_betas(100), time_scale=100).respace([0, 5, 15, 30, 50, 70, 90]).with_learned_variance()
        assert [r.time(k) for k in range(r.Ns)] == [0.0, 5.0, 15.0, 30.0, 50.0, 70.0, 90.0]
    assert r.Ns == 7
    x0, cond, noise = _data()
    amortized = case.startswith("amortized")
    net = nets["labels"] if case == "labels" else nets[(2, 2) if amortized else (1, 2)]
    y = torch.tensor([3, 0, 2], device=DEV) if case == "labels" else None
    cnd = cond if case == "amortized" else None
    philox = case == "plain_philox_tanh_unclipped"
    cdf, clip = ("tanh", False) if philox else ("exact", True)
    vlb = bound.get_vlb_fn(sampling.make_eps_model(net, r), r, Amortized(1.0, 0, 0.1) if amortized else None, lik if amortized else None, cdf=cdf,
                           clip_denoised=clip)
    kw = dict(condition=None if cnd is None else cnd.to(DEV), y=y)
    res = vlb(x0.to(DEV), noise=None if philox else noise.to(DEV), seed=991 if philox else None, **kw)
    got = _as_dict(res)
    logs = r.vlb_log_variances("learned")
    draws = noise
    if philox:   # the draws the loop used, fetched at the same (seed, offset)
        n_al = (x0.numel() + 3) // 4 * 4
        draws = torch.stack([ops.randn(tuple(x0.shape), DEV, 991, j * n_al).cpu() for j in range(r.Ns)])
    terms, summary = _host_loop(net, r, logs, x0.to(DEV), None if philox else noise.to(DEV), learned=True, cond=None if cnd is None else cnd.to(DEV), y=y,
                                seed=991, cdf=cdf, clip=clip)
    host = dict(total_bpd=summary[:, 1].cpu(), prior_bpd=summary[:, 0].cpu(), vb=terms[:, :, 0].cpu(), xstart_mse=terms[:, :, 1].cpu(), mse=terms[:, :, 2].cpu())
    for f in FIELDS:
        d = float((got[f].double() - host[f].double()).abs().max())
        print(f"{case}: {f}: fused vs host loop of ops, max |diff| {d:.3e}")
    for f in FIELDS:
        assert torch.equal(_bits(got[f]), _bits(host[f])), f"{case}: {f}: the fused loop and the host loop of ops differ"
    ref = VR.loop(_net_out(net, r, y), r.host_tables(), logs, x0, draws, learned=True, cdf=cdf, clip=clip, cond=cnd, amortized=amortized)
    _close(case, got, ref)
    # the variance channels matter: the same net's eps channels under the fixed posterior variance give another bound
    fixed_logs = r.vlb_log_variances("fixed_small")
    fixed = VR.loop(_net_out(net, r, y), r.host_tables(), fixed_logs, x0, draws, learned=False, cdf=cdf, clip=clip, cond=cnd, amortized=amortized)
    ft, fs = _host_loop(net, r, fixed_logs, x0.to(DEV), None if philox else noise.to(DEV), learned=False, cond=None if cnd is None else cnd.to(DEV), y=y,
                        seed=991, cdf=cdf, clip=clip)
    torch.testing.assert_close(fs[:, 1].cpu().double(), torch.from_numpy(fixed["total_bpd"]), **STOL)
    gap = (got["total_bpd"].double() - torch.from_numpy(fixed["total_bpd"])).abs()
    margin = STOL["atol"] + STOL["rtol"] * torch.from_numpy(np.abs(fixed["total_bpd"]))
    print(f"{case}: total_bpd learned {got['total_bpd'].tolist()} vs fixed_small {fixed['total_bpd'].tolist()}")
    assert bool((gap > margin).all()), "the learned variance does not move the bound: the test shows nothing"
    # the parts add up, and the decoder / KL columns are where they belong
    total = (got["vb"].double().sum(1) + got["prior_bpd"].double()).float()
    assert float((got["total_bpd"] - total).abs().max()) <= float(np.spacing(np.float32(total.abs().max())))
    net.engine(DEV).check()


# ---- 3. a 3-output net ------------------------------------------------------------------------------------------------------------------------------------

def test_fixed_variances_on_a_three_output_net(nets):
    from image_diffusion import bound, sampling

    r = _chain()
    net = nets[(3, 3)]
    x0, _, noise = _data(3)
    out = {}
    for variance in ("fixed_small", "fixed_large"):
        vlb = bound.get_vlb_fn(sampling.make_eps_model(net, r), r, variance=variance)
        out[variance] = _as_dict(vlb(x0.to(DEV), noise=noise.to(DEV)))
        ref = VR.loop(_net_out(net, r), r.host_tables(), r.vlb_log_variances(variance), x0, noise, learned=False)
        _close(variance, out[variance], ref)
    default = _as_dict(bound.get_vlb_fn(sampling.make_eps_model(net, r), r)(x0.to(DEV), noise=noise.to(DEV)))
    assert all(torch.equal(_bits(default[f]), _bits(out["fixed_small"][f])) for f in FIELDS), "variance=None on a plain chain is fixed_small"
    a, b = out["fixed_small"]["total_bpd"].double(), out["fixed_large"]["total_bpd"].double()
    print(f"3-output net: total_bpd fixed_small {a.tolist()} fixed_large {b.tolist()}")
    assert bool(((a - b).abs() > STOL["atol"] + STOL["rtol"] * b.abs()).all())
    # the diagnostics do not depend on the variance
    for f in ("prior_bpd", "xstart_mse", "mse"):
        assert torch.equal(_bits(out["fixed_small"][f]), _bits(out["fixed_large"][f])), f
    net.engine(DEV).check()


# ---- 4. identities -------------------------------------------------------------------------------------------------------------------------------------------

def test_identities_that_need_no_reference(nets):
    from image_diffusion import bound, sampling
    from mi355.ops import default_ops as ops

    r = _chain()
    T = r.host_tables()
    K = r.Ns
    x0, _, noise = _data()
    # a net that writes zeros, unclipped: mse = mean(z_k^2), xstart_mse = mean((c_recip x_k - x0)^2), each the fp64 value rounded once
    res = _as_dict(bound.get_vlb_fn(sampling.make_eps_model(nets["zero"], r), r, clip_denoised=False)(x0.to(DEV), noise=noise.to(DEV)))
    for k in range(K):
        z = noise[K - 1 - k].numpy()
        xk = VR.q_sample32(x0.numpy(), z, T["sqrt_alphas_cumprod"][k].item(), T["sqrt_one_minus_alphas_cumprod"][k].item())
        mz = (z.astype(np.float64) ** 2).reshape(B, -1).mean(1)
        mx = ((float(T["sqrt_recip_alphas_cumprod"][k]) * xk.astype(np.float64) - x0.numpy().astype(np.float64)) ** 2).reshape(B, -1).mean(1)
        for name, want in (("mse", mz), ("xstart_mse", mx)):
            got = res[name][:, k].double().numpy()
            assert (np.abs(got - want) <= (1 + 1e-6) * EPS32 * np.abs(want)).all(), (name, k, got, want)
    # a real net: the mse column is mse_per_sample(eps, z_k).  That kernel rounds the difference to fp32 before squaring (2 EPS32 on the square),
    # both outputs are rounded once (EPS32 each); fp64 accumulation on both sides
    net = nets[(1, 1)]
    res = _as_dict(bound.get_vlb_fn(sampling.make_eps_model(net, r), r)(x0.to(DEV), noise=noise.to(DEV)))
    eng = net.engine(DEV)
    for k in range(K):
        z = noise[K - 1 - k].to(DEV)
        xk = ops.q_sample(x0.to(DEV), float(T["sqrt_alphas_cumprod"][k]), float(T["sqrt_one_minus_alphas_cumprod"][k]), z=z)
        want = ops.mse_per_sample(eng.forward(xk, r.time(k)), z).cpu().double()
        got = res["mse"][:, k].double()
        assert bool(((got - want).abs() <= 5 * EPS32 * want.abs()).all()), (k, got, want)
    eng.check()


# ---- 5. one library call per batch ------------------------------------------------------------------------------------------------------------------------------

def test_public_path_is_one_library_call(nets, monkeypatch):
    from image_diffusion import bound, sampling
    from mi355 import _lib

    r = _chain().with_learned_variance()
    net = nets[(1, 2)]
    eng = net.engine(DEV)
    x0, _, _ = _data()
    # what one evaluation inside a fused DDPM loop launches on this net: the learned-variance sampler reports it with its one step launch
    eng.ddpm_learned(x0.to(DEV).clone(), r.host_tables(), r.max_log(), mode=_lib.DDPM_PRIOR, timesteps=r.timesteps, train_steps=r.base_Ns)
    n_eval = eng.stats(B)["launches"] - 1
    calls = []
    real = eng.ddpm_vlb
    monkeypatch.setattr(eng, "ddpm_vlb", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(eng, "forward", lambda *a, **k: pytest.fail("a forward outside the fused loop ran"))
    res = bound.get_vlb_fn(sampling.make_eps_model(net, r), r)(x0.to(DEV))
    assert len(calls) == 1 and n_eval > 0 and eng.stats(B)["launches"] == n_eval + 2, (len(calls), eng.stats(B)["launches"], n_eval)
    assert all(bool(torch.isfinite(getattr(res, f)).all()) for f in FIELDS) and tuple(res.vb.shape) == (B, r.Ns) and tuple(res.total_bpd.shape) == (B,)
    # device Philox: the same seed gives the same bits, another seed another bound
    again = bound.get_vlb_fn(sampling.make_eps_model(net, r), r)(x0.to(DEV))
    other = bound.get_vlb_fn(sampling.make_eps_model(net, r), r)(x0.to(DEV), seed=12345)
    assert torch.equal(_bits(res.vb), _bits(again.vb)) and not torch.equal(_bits(res.vb), _bits(other.vb))
    eng.check()


# ---- 6. the refusals that need a handle ------------------------------------------------------------------------------------------------------------------------

def test_refusals_that_need_a_handle(nets):
    from mi355 import _lib
    from mi355._lib import MI355BackendError

    r = _chain().with_learned_variance()
    T = r.host_tables()
    learned, fixed = r.vlb_log_variances("learned"), r.vlb_log_variances("fixed_small")
    x0, cond, noise = (t.to(DEV) for t in _data())
    L = _lib.lib()
    narrow, wide, wide2 = nets[(1, 1)].engine(DEV), nets[(1, 2)].engine(DEV), nets[(2, 2)].engine(DEV)
    cases = [(narrow, dict(logs=learned, learned=True), "opt->learned needs a net whose out_channels == 2 \\* channels"),
             (wide, dict(logs=fixed, learned=False), "needs a net whose out_channels == channels"),
             (wide, dict(logs=learned, learned=True, cond=cond), "cond given to a net that takes no condition"),
             (wide, dict(logs=learned, learned=True, noise=noise[:3].contiguous()), "injected noise exhausted")]
    for eng, kw, msg in cases:
        before = eng.stats(B)["launches"]
        with pytest.raises(MI355BackendError, match="ddpm_vlb: .*" + msg):
            eng.ddpm_vlb(x0, T, **kw)
        assert b"ddpm_vlb" in L.mi355_last_error() and eng.stats(B)["launches"] == before
    with pytest.raises(ValueError, match="built without num_classes"):
        wide.ddpm_vlb(x0, T, learned, learned=True, y=torch.tensor([0, 1, 2], device=DEV))
    # through the ABI, with outputs that must stay as they are: labels on a net without classes, a short workspace, a missing output
    tb, keep = wide._ddpm_tables(T)
    fp = C.POINTER(C.c_float)
    opt = _lib.VLBOptionsC(1, 0, 1, *(C.cast(learned[n].data_ptr(), fp) for n in ("true_log", "true_log", "min_log", "max_log")), None, -2.0, 0)
    terms, summary = torch.full((B, r.Ns, 3), 7.0, device=DEV), torch.full((B, 2), 7.0, device=DEV)
    labels = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    ws, wsb = wide._workspace_sized("mi355_ddpm_vlb_workspace_bytes", B)
    assert wsb >= L.mi355_unet_workspace_bytes(wide.handle, B) > 0

    def call(eng, lab=None, ws=ws, wsb=wsb, out=terms):
        return L.mi355_ddpm_vlb(eng.handle, C.c_void_p(x0.data_ptr()), 1, None, C.c_void_p(lab.data_ptr()) if lab is not None else None, C.byref(tb),
                                C.byref(opt), None, 0, C.c_void_p(out.data_ptr()) if out is not None else None, C.c_void_p(summary.data_ptr()), B, ws, wsb,
                                None)

    assert call(wide, lab=labels) == -1 and b"ddpm_vlb: labels given to a net built without num_classes" in L.mi355_last_error()
    assert call(wide, wsb=4096) == -2 and b"ddpm_vlb: workspace too small" in L.mi355_last_error()
    assert call(wide, out=None) == -1 and b"ddpm_vlb: out_terms is null" in L.mi355_last_error()
    assert call(wide2, ws=None) == -1 and b"ddpm_vlb: workspace is null" in L.mi355_last_error()
    torch.cuda.synchronize()
    assert bool((terms == 7.0).all()) and bool((summary == 7.0).all()), "a refused call launched something"
    # the Python layer's own
    with pytest.raises(ValueError, match="is needed"):
        wide.ddpm_vlb(x0, T, fixed, learned=True)
    with pytest.raises(ValueError, match="one entry per row"):
        wide.ddpm_vlb(x0, T, {k: v[:3] for k, v in learned.items()}, learned=True)
    with pytest.raises(ValueError, match="noise must be"):
        wide.ddpm_vlb(x0, T, learned, learned=True, noise=noise[:, :2].contiguous())
    from image_diffusion import bound, sampling

    with pytest.raises(ValueError, match="twice the data's channels"):
        bound.get_vlb_fn(sampling.make_eps_model(nets[(1, 1)], r), r)(x0)
    with pytest.raises(ValueError, match='variance "fixed_small" needs the data\'s channels'):
        bound.get_vlb_fn(sampling.make_eps_model(nets[(1, 2)], r), r, variance="fixed_small")(x0)
    with pytest.raises(ValueError, match="a condition needs Amortized"):
        bound.get_vlb_fn(sampling.make_eps_model(nets[(1, 2)], r), r)(x0, condition=cond)
    from mi355.ops import default_ops as ops

    with pytest.raises(ValueError, match="twice the state's channels"):
        ops.vlb_terms(x0, x0, x0, c_recip=1.0, c_recipm1=0.5, coef1=0.5, coef2=0.5, true_log=-3.0, min_log=-3.0, max_log=-1.0, k_is_zero=False,
                      learned=True, z=x0)
    with pytest.raises(MI355BackendError, match="vlb_terms: the step's draw is needed"):
        ops.vlb_terms(x0, x0, x0, c_recip=1.0, c_recipm1=0.5, coef1=0.5, coef2=0.5, true_log=-3.0, model_log=-3.0, k_is_zero=False, learned=False)
    with pytest.raises(MI355BackendError, match="q_sample: out must not be x0"):
        ops.q_sample(x0, 0.5, 0.5, z=x0, out=x0)
    del keep
    wide.check()


# ---- 7. the denoising loss and the evaluation loop ------------------------------------------------------------------------------------------------------------

def test_get_loss_function(nets):
    from image_diffusion.conditioning import Amortized, Replacement
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.loss_functions import get_loss_function

    r = _chain()
    T = r.host_tables()
    lik = InPainting(patch_size=4, pad_value=-2)
    x0, _, noise = _data()
    i = torch.tensor([6, 0, 3])
    xd = x0.to(DEV)

    def out_fn(net):
        def out(net_in, steps):
            t = torch.tensor([r.time(int(k)) for k in steps], dtype=torch.float32, device=DEV)
            return net(net_in.to(DEV).contiguous(), t).cpu()
        return out

    loss, eps_model = get_loss_function(nets[(1, 1)], r, Replacement(0.1, 1.0, True, 0), lik)
    got = float(loss(xd, i=i.to(DEV), noise=noise[0].to(DEV)))
    want = VR.loss(out_fn(nets[(1, 1)]), T, x0, i, noise[0])
    print(f"generic loss: {got:.6f} vs fp64 {want:.6f}")
    assert abs(got - want) <= STOL["atol"] + STOL["rtol"] * abs(want)
    assert eps_model._mi355_network is nets[(1, 1)]
    aloss, _ = get_loss_function(nets[(2, 1)], r, Amortized(0.5, 0, 0.1), lik)
    for use in (True, False):
        torch.manual_seed(5)
        cond = (lik.sample(xd) if use else lik.none_like(xd)).cpu()
        torch.manual_seed(5)
        got = float(aloss(xd, i=i.to(DEV), noise=noise[1].to(DEV), use_condition=use))
        want = VR.loss(out_fn(nets[(2, 1)]), T, x0, i, noise[1], cond=cond)
        print(f"amortized loss (use_condition = {use}): {got:.6f} vs fp64 {want:.6f}")
        assert abs(got - want) <= STOL["atol"] + STOL["rtol"] * abs(want)
    # the draws left to their defaults: the same torch seed, the same number
    for fn in (loss, aloss):
        torch.manual_seed(77)
        a = float(fn(xd))
        torch.manual_seed(77)
        b = float(fn(xd))
        torch.manual_seed(78)
        c = float(fn(xd))
        assert a == b and a != c and np.isfinite(a)
    assert not aloss(xd).requires_grad


def test_evaluate_writes_the_bpd_column(nets, tmp_path):
    import evaluation
    from image_diffusion import bound, sampling
    from image_diffusion.likelihoods import InPainting

    r = _chain().with_learned_variance()
    lik = InPainting(patch_size=4, pad_value=-2)
    x0 = _data()[0].to(DEV)
    vlb = bound.get_vlb_fn(sampling.make_eps_model(nets[(1, 2)], r), r)
    sample_fn = lambda xT, cond: (0.5 * xT).clamp(-1, 1)   # noqa: E731  (the loop's plumbing is what is under test)
    runs = {}
    for name, kw in (("parent", {}), ("none", dict(vlb_fn=None)), ("bpd", dict(vlb_fn=vlb, metrics=("mse", "bpd"))),
                     ("bpd_no_fn", dict(metrics=("mse", "bpd")))):
        torch.manual_seed(31)
        out = evaluation.evaluate(sample_fn, lik, [x0, x0.flip(0)], tmp_path / name, save_images=False, **kw)
        runs[name] = (out, (tmp_path / name / "results.json").read_text())
        assert json.loads(runs[name][1]) == out
    assert runs["none"][1] == runs["parent"][1] and "bpd" not in runs["parent"][1]
    torch.manual_seed(31)
    want = torch.cat((vlb(x0).total_bpd, vlb(x0.flip(0)).total_bpd))
    out = runs["bpd"][0]
    assert list(out) == ["mse_mean", "bpd_mean", "mse_median", "bpd_median", "mse_std", "bpd_std", "fid"]
    assert out["bpd_mean"] == torch.mean(want).item() and out["bpd_median"] == torch.median(want).item() and out["bpd_std"] == torch.std(want).item()
    assert out["mse_mean"] == json.loads(runs["parent"][1])["mse_mean"]
    assert runs["bpd_no_fn"][0]["bpd_mean"] is None
