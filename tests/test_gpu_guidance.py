"""GPU: the U-Net data gradient (mi355_unet_vjp) and the reconstruction-guidance sampler (AD/image_diffusion/sampling.py:136-206)
against vectors produced by the reference's own UNetModel / DDPM / likelihood.loss under torch.autograd / torch.func.vmap(grad)
(tools/make_goldens.py g_unet_vjp, g_recon_guidance) and against the CPU oracle at the CIFAR configuration.

Tolerances: fp32 mode; a gradient is compared relative to its largest entry (rtol 2e-3, atol 5e-4 * max|ref|); samplers as the
other 25-step DDPM samplers (rtol 2e-3, atol 1e-3).  bf16 mode: every image's gradient against the fp32 oracle, relative rms error
(||err|| / ||ref||) and max|err| / max|ref| per image, bounds set at about 3x the worst values measured on the MI355X (_check_bf16_images)."""
import time

import numpy as np
import pytest
import torch

from mi355.synth import rand_uniform, randn, synth_state_dict
from oracle import ddpm_ref, unet_ref
from tests.test_oracle_golden import NoiseLog, cfg_from_json

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _build(cfg, seed, precision="fp32", **kw):
    from image_diffusion.unet import UNetModel, param_shapes

    net = UNetModel(image_size=cfg.image_size, in_channels=cfg.in_channels, model_channels=cfg.model_channels,
                    out_channels=cfg.out_channels, num_res_blocks=cfg.num_res_blocks, attention_resolutions=cfg.attention_resolutions,
                    channel_mult=cfg.channel_mult, conv_resample=cfg.conv_resample, num_heads=cfg.num_heads,
                    num_head_channels=cfg.num_head_channels, num_heads_upsample=cfg.num_heads_upsample,
                    use_scale_shift_norm=cfg.use_scale_shift_norm, resblock_updown=cfg.resblock_updown,
                    use_new_attention_order=cfg.use_new_attention_order, precision=precision, **kw)
    sd = synth_state_dict(param_shapes(cfg), seed)
    net.load_state_dict(sd)
    return net.to(DEV), sd


def _close_grad(got, ref, rtol=2e-3, rel_atol=5e-4):
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"   grad max|err| {err:.3e} (max|ref| {scale:.3e})")
    torch.testing.assert_close(got, ref, rtol=rtol, atol=rel_atol * scale)


def _oracle_vjp(sd, cfg, x, t, cot):
    """(d out / d x)^T cot of the fp32 oracle under torch.autograd."""
    xr = x.clone().requires_grad_()
    (g,) = torch.autograd.grad((unet_ref.unet_forward_diff(sd, cfg, xr, t) * cot).sum(), xr)
    return g


def _check_bf16_images(got, ref, rms_bound, max_bound, tag):
    """bf16 VJP against the fp32 oracle, image by image: relative rms error and max|err| / max|ref| of each image."""
    assert torch.isfinite(got).all(), tag
    dims = tuple(range(1, ref.dim()))
    rms = (got - ref).pow(2).mean(dim=dims).sqrt() / ref.pow(2).mean(dim=dims).sqrt()
    mx = (got - ref).abs().amax(dim=dims) / ref.abs().amax(dim=dims)
    print(f"   {tag} bf16: worst per-image relative rms {float(rms.max()):.3e} (bound {rms_bound}), "
          f"worst per-image max|err|/max|ref| {float(mx.max()):.3e} (bound {max_bound})")
    assert float(rms.max()) < rms_bound, (tag, rms.tolist())
    assert float(mx.max()) < max_bound, (tag, mx.tolist())


# Synthetic-weight nets whose differentiable plans reach the attention-backward head sizes the goldens do not (96, 128, 192, 256), attention
# at 4x4 (T = 16) and the new channel order above 64 head channels; 16-px images, attention at ds 1 (T = 256), 2 (T = 64) or 4 (T = 16).
VJP_SYNTH = {
    "ch96_192": unet_ref.UNetConfig(16, 3, 96, 3, 1, (1, 2), channel_mult=(1, 2), num_heads=1),
    "ch128_256_neworder": unet_ref.UNetConfig(16, 3, 128, 3, 1, (1, 2), channel_mult=(1, 2), num_heads=1, use_new_attention_order=True),
    "t16_heads2": unet_ref.UNetConfig(16, 3, 32, 3, 1, (4,), channel_mult=(1, 2, 2), num_heads=2),
}
# bf16 bounds per image vs the fp32 oracle, (relative rms, max|err| / max|ref|): about 3x the worst image measured on the MI355X, which was
# ch96_192 (1.41e-2, 1.38e-2), ch128_256_neworder (1.31e-2, 1.42e-2), t16_heads2 (2.32e-2, 2.44e-2), cifar (1.25e-2, 1.72e-2)
SYNTH_BF16 = {"ch96_192": (0.045, 0.045), "ch128_256_neworder": (0.04, 0.045), "t16_heads2": (0.07, 0.075)}
CIFAR_BF16_RMS, CIFAR_BF16_MAX = 0.04, 0.05


def _synth_case(name, idx):
    cfg = VJP_SYNTH[name]
    B = 5                                                           # not a power of two; a distinct t per image
    x = randn(400 + idx, B, cfg.in_channels, cfg.image_size, cfg.image_size)
    t = torch.tensor([0.03, 0.27, 0.5, 0.71, 0.96])
    cot = randn(410 + idx, B, cfg.out_channels, cfg.image_size, cfg.image_size)
    return cfg, 2000 + idx, x, t, cot


@pytest.mark.parametrize("name", list(VJP_SYNTH))
def test_unet_vjp_synth_configs(name):
    """Every image of a batch of 5 against the oracle's autograd, fp32 at the golden tolerances and bf16 at the measured bounds (SYNTH_BF16)."""
    idx = list(VJP_SYNTH).index(name)
    cfg, seed, x, t, cot = _synth_case(name, idx)
    net, sd = _build(cfg, seed)
    ref = _oracle_vjp(sd, cfg, x, t, cot)
    eng = net.engine(DEV, differentiable=True)
    eng.forward(x.to(DEV), t.to(DEV))
    _close_grad(eng.vjp(cot.to(DEV)).cpu(), ref)
    net.set_precision("bf16")
    eng = net.engine(DEV, differentiable=True)
    eng.forward(x.to(DEV), t.to(DEV))
    _check_bf16_images(eng.vjp(cot.to(DEV)).cpu(), ref, *SYNTH_BF16[name], name)


def test_use_fp16_model_is_differentiable_in_bf16():
    """use_fp16=True selects precision 'fp16', which has no backward pass: the differentiable plan is built in bf16 (bf16x2 likewise), the
    plain engine keeps fp16, and the VJP meets the bf16 bounds against the oracle."""
    name = "t16_heads2"
    cfg, seed, x, t, cot = _synth_case(name, list(VJP_SYNTH).index(name))
    net, sd = _build(cfg, seed, precision=None, use_fp16=True)
    assert net.precision == "fp16"
    deng = net.engine(DEV, differentiable=True)
    assert deng.precision == "bf16" and net.engine(DEV).precision == "fp16"
    deng.forward(x.to(DEV), t.to(DEV))
    _check_bf16_images(deng.vjp(cot.to(DEV)).cpu(), _oracle_vjp(sd, cfg, x, t, cot), *SYNTH_BF16[name], "use_fp16")
    assert net.set_precision("bf16x2").engine(DEV, differentiable=True).precision == "bf16"


def test_reconstruction_guidance_on_a_use_fp16_model(golden):
    """The golden's guided sample ("paint_before": 25 steps, every one guided) on the same tiny net built with use_fp16=True runs (guided
    steps on the bf16 differentiable plan) and stays finite and near the fp32 reference's result (measured max|err| 0.23; the bound only
    rejects garbage)."""
    from image_diffusion import sampling
    from image_diffusion.conditioning import ReconstructionGuidance
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM

    g = golden("recon_guidance_tiny")
    ddpm = DDPM(int(g["Ns"]))
    cfg = unet_ref.UNetConfig(16, 1, 32, 1, 1, (2,), channel_mult=(1, 2), num_heads=2)
    net, _ = _build(cfg, int(g["net_seed"]), precision=None, use_fp16=True)
    tag = "paint_before"
    cond = ReconstructionGuidance(float(g[f"{tag}/gamma"]), float(g[f"{tag}/start_fraction"]), str(g[f"{tag}/rule"]), int(g[f"{tag}/n_corrector"]), 0.1)
    shape = tuple(g[f"{tag}/xT"].shape)
    base, k = int(g[f"{tag}/noise_base"]), int(g[f"{tag}/draws"])
    with sampling.injected_noise([randn(base + j, *shape) for j in range(k)]):
        x0 = sampling.get_conditional_sample_fn(sampling.make_eps_model(net, ddpm), ddpm, cond, InPainting(6, -2))(
            g.t(f"{tag}/xT").to(DEV), g.t(f"{tag}/cond").to(DEV)).cpu()
    assert torch.isfinite(x0).all()
    err = float((x0 - g.t(f"{tag}/x0")).abs().max())
    print(f"   use_fp16 guided sample: max|err| vs the fp32 reference {err:.3e}")
    assert err < 0.5   # x0 lies in [-1, 1]: a loose bound that garbage would not meet
    assert net.engine(DEV).precision == "fp16" and net.engine(DEV, differentiable=True).precision == "bf16"


def test_differentiable_plan_refuses_head_channels_above_256():
    """The attention backward has head sizes up to 256: a differentiable plan with 384 head channels fails when the engine is built,
    with the reason, not in the middle of a guided sample; the forward-only plan of the same net builds."""
    from mi355._lib import MI355BackendError

    cfg = unet_ref.UNetConfig(8, 3, 384, 3, 1, (1,), channel_mult=(1,), num_heads=1)
    net, _ = _build(cfg, 5, precision="bf16")
    with pytest.raises(MI355BackendError, match="up to 256"):
        net.engine(DEV, differentiable=True)
    net.engine(DEV)


@pytest.mark.parametrize("name", ["tiny_in1", "tiny_in3", "tiny_film_updown_neworder", "tiny_noconvresample", "mnist", "cifar", "flowers_in3"])
def test_unet_vjp_vs_reference_autograd(golden, name):
    """(d out / d x)^T g of the differentiable plan against the reference UNetModel under torch.autograd: plain / FiLM / up-down
    ResBlocks, conv and pool resampling, both attention orders, skip concats, 1x1 and 3x3 skips, stride-2 and nearest-x2 convs."""
    g = golden("unet_vjp")
    cfg = cfg_from_json(g.json(f"{name}/config"))
    net, _ = _build(cfg, int(g[f"{name}/seed"]))
    eng = net.engine(DEV, differentiable=True)
    x, t, cot = g.t(f"{name}/x").to(DEV), g.t(f"{name}/t").to(DEV), g.t(f"{name}/g").to(DEV)
    y = eng.forward(x, t)
    torch.testing.assert_close(y.cpu(), g.t(f"{name}/y"), rtol=2e-4, atol=5e-5)   # the differentiable plan's forward is the same network
    gx = eng.vjp(cot, x_channels=cfg.in_channels)
    _close_grad(gx.cpu(), g.t(f"{name}/gx"))
    # linearity in the cotangent and repeatability (the backward pass reads, never destroys, the kept activations)
    gx2 = eng.vjp((2.0 * cot).contiguous(), x_channels=cfg.in_channels)
    torch.testing.assert_close(gx2, 2.0 * gx, rtol=1e-4, atol=1e-5 * float(gx.abs().max()))


def test_unet_vjp_cifar_batch_vs_oracle():
    """A larger batch of the CIFAR net (so the big-tile / persistent conv kernels run the data-gradient convs too): oracle autograd
    on all 64 images (in chunks of 16; about 1 s on 16 CPU cores), fp32 and bf16 mode; bf16 per image at CIFAR_BF16_RMS / _MAX and the
    whole batch's relative rms below 5 %."""
    kw = dict(image_size=32, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(2,),
              channel_mult=(1, 2, 2, 2), num_heads=4, num_head_channels=64)
    cfg = unet_ref.UNetConfig(32, 3, 128, 3, 2, (2,), channel_mult=(1, 2, 2, 2), num_heads=4, num_head_channels=64)
    net, sd = _build(cfg, 1234)
    B = 64
    x, t, cot = randn(31, B, 3, 32, 32), torch.linspace(0.05, 0.95, B), randn(32, B, 3, 32, 32)
    eng = net.engine(DEV, differentiable=True)
    eng.forward(x.to(DEV), t.to(DEV))
    gx = eng.vjp(cot.to(DEV)).cpu()
    t0 = time.perf_counter()
    ref = torch.cat([_oracle_vjp(sd, cfg, x[i:i + 16], t[i:i + 16], cot[i:i + 16]) for i in range(0, B, 16)])
    print(f"   oracle VJP of {B} images: {time.perf_counter() - t0:.1f} s")
    _close_grad(gx, ref)
    net.set_precision("bf16")
    eng = net.engine(DEV, differentiable=True)
    eng.forward(x.to(DEV), t.to(DEV))
    g16 = eng.vjp(cot.to(DEV)).cpu()
    rel = float((g16 - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"   bf16 vjp relative rms error {rel:.3e} (whole batch)")
    assert torch.isfinite(g16).all() and rel < 0.05
    _check_bf16_images(g16, ref, CIFAR_BF16_RMS, CIFAR_BF16_MAX, "cifar")


def test_guidance_gradient_probes(golden):
    """x_grad = vmap(grad(constraint))(xi, i, y) at fixed points: seed kernel (loss, clip, predict_start chain rule) + U-Net VJP."""
    from image_diffusion.sde_diffusion import DDPM
    from mi355.ops import default_ops as ops

    g = golden("recon_guidance_tiny")
    Ns = int(g["Ns"])
    cfg = unet_ref.UNetConfig(16, 1, 32, 1, 1, (2,), channel_mult=(1, 2), num_heads=2)
    net, _ = _build(cfg, int(g["net_seed"]))
    eng = net.engine(DEV, differentiable=True)
    T = DDPM(Ns).host_tables()
    for lname, mode in (("paint", 0), ("hyper", 1)):
        cond = g.t(f"probe/{lname}/cond").to(DEV)
        for i in (18, 12, 3):
            xi = g.t(f"probe/{lname}/i{i}/xi").to(DEV)
            eps = eng.forward(xi, torch.full((xi.shape[0],), i / Ns, device=DEV))
            g_eps, g_x = ops.guidance_seed(xi, eps, cond, float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i]),
                                           mode, -2.0)
            x_grad = (g_x + eng.vjp(g_eps)).cpu()
            _close_grad(x_grad, g.t(f"probe/{lname}/i{i}/grad"))


def test_reconstruction_guidance_sampler_golden(golden):
    """get_conditional_sample_fn[ReconstructionGuidance] against the reference-driven golden: both update rules, start_fraction,
    a corrector step, Painting.loss and HyperResolution.loss."""
    from image_diffusion import sampling
    from image_diffusion.conditioning import ReconstructionGuidance
    from image_diffusion.likelihoods import HyperResolution, InPainting
    from image_diffusion.sde_diffusion import DDPM

    g = golden("recon_guidance_tiny")
    Ns = int(g["Ns"])
    ddpm = DDPM(Ns)
    cfg = unet_ref.UNetConfig(16, 1, 32, 1, 1, (2,), channel_mult=(1, 2), num_heads=2)
    net, _ = _build(cfg, int(g["net_seed"]))
    eps = sampling.make_eps_model(net, ddpm)
    for tag in ("paint_before", "paint_after", "paint_half_corr1", "hyper_before"):
        lik = InPainting(6, -2) if str(g[f"{tag}/loss"]) == "painting" else HyperResolution(4, 4)
        cond = ReconstructionGuidance(float(g[f"{tag}/gamma"]), float(g[f"{tag}/start_fraction"]), str(g[f"{tag}/rule"]),
                                      int(g[f"{tag}/n_corrector"]), 0.1)
        shape = tuple(g[f"{tag}/xT"].shape)
        base, k = int(g[f"{tag}/noise_base"]), int(g[f"{tag}/draws"])
        with sampling.injected_noise([randn(base + j, *shape) for j in range(k)]):
            x0 = sampling.get_conditional_sample_fn(eps, ddpm, cond, lik)(g.t(f"{tag}/xT").to(DEV), g.t(f"{tag}/cond").to(DEV))
        err = float((x0.cpu() - g.t(f"{tag}/x0")).abs().max())
        print(f"   {tag}: max|err| {err:.3e}")
        torch.testing.assert_close(x0.cpu(), g.t(f"{tag}/x0"), rtol=2e-3, atol=1e-3)
    # an arbitrary callable has no backward pass on this backend: loud error, no fallback
    with pytest.raises(NotImplementedError):
        sampling.get_conditional_sample_fn(lambda xi, i: net(xi, 1.0 * i / Ns), ddpm, ReconstructionGuidance(1.0, 1.0, "before", 0, 0.1),
                                           InPainting(6, -2))
