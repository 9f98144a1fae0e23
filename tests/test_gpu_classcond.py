"""GPU: class-conditional U-Nets on the HIP path - the label term emb = time_embed(timestep_embedding(t)) + label_emb(y) (upstream
guided-diffusion / torchcfm rule) in the single forward, the Euler sampler (its (step, class) table path and its per-step fallback), the
dopri5 sampler of conditional_mnist.ipynb and the data gradient.

There is no reference fixture for the label path: the reference's forward never adds label_emb (AD/image_diffusion/unet.py:708-728)
and torchcfm is not vendored.  The expectation is tests/test_classcond_cpu.classcond_forward, an fp32 restatement composed of
oracle.unet_ref's pieces; the y=None behaviour is pinned by the reference fixtures tests/golden/unet_*_classcond.npz.

Tolerances: fp32 as the whole-net forward (rtol 2e-4, atol 5e-5); bf16 / fp16 / bf16x2 the bounds of test_gpu_configs.py.
"""
import pytest
import torch

from mi355.synth import randn, synth_state_dict
from oracle import cfm_ref
from tests.test_classcond_cpu import CLASSCOND, ClassCondConfig, classcond_forward, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(cfg, seed, precision, sd=None):
    from image_diffusion.unet import UNetModel, param_shapes

    net = UNetModel(image_size=cfg.image_size, in_channels=cfg.in_channels, model_channels=cfg.model_channels,
                    out_channels=cfg.out_channels, num_res_blocks=cfg.num_res_blocks, attention_resolutions=cfg.attention_resolutions,
                    channel_mult=cfg.channel_mult, conv_resample=cfg.conv_resample, num_heads=cfg.num_heads,
                    num_head_channels=cfg.num_head_channels, num_heads_upsample=cfg.num_heads_upsample,
                    use_scale_shift_norm=cfg.use_scale_shift_norm, resblock_updown=cfg.resblock_updown,
                    use_new_attention_order=cfg.use_new_attention_order, num_classes=cfg.num_classes, precision=precision)
    if sd is None:
        sd = synth_state_dict(param_shapes(cfg), seed)
    net.load_state_dict(sd)
    return net.to(DEV), sd


def _report(tag, got, ref):
    err = (got - ref).abs()
    scale = ref.abs().max().item()
    rms = err.pow(2).mean().sqrt().item() / max(ref.pow(2).mean().sqrt().item(), 1e-12)
    print(f"{tag}: max|err| {err.max().item():.3e} (scale {scale:.3f}), rel rms {rms:.3e}")
    return err.max().item(), scale, rms


def _labels(case, B, K):
    return torch.tensor([(3 * case + 2 * b + 1) % K for b in range(B)], dtype=torch.int64)


MNIST_NB = ClassCondConfig(28, 1, 32, 1, 1, (1,), channel_mult=(1, 2, 2), num_classes=10)   # conditional_mnist.ipynb's wrapper


@pytest.mark.parametrize("shared_t", [False, True])
@pytest.mark.parametrize("name", CLASSCOND)
def test_forward_fp32_vs_restatement(golden, name, shared_t):
    g, cfg = load_case(golden, name)
    net, sd = _model(cfg, int(g["seed"]), "fp32")
    x = g.t("x")
    B = x.shape[0]
    y = _labels(CLASSCOND.index(name), B, cfg.num_classes)
    t = torch.full((B,), 0.42) if shared_t else g.t("t")
    ref = classcond_forward(sd, cfg, x, t, y)
    eng = net.engine(DEV)
    got = eng.forward(x.to(DEV), 0.42, y=y.to(DEV)) if shared_t else net(x.to(DEV), t.to(DEV), y.to(DEV))
    torch.testing.assert_close(got.cpu(), ref, rtol=2e-4, atol=5e-5)
    eng.check()


@pytest.mark.parametrize("precision", ["bf16", "fp16", "bf16x2"])
@pytest.mark.parametrize("name", CLASSCOND)
def test_forward_reduced_precision_vs_restatement(golden, name, precision):
    g, cfg = load_case(golden, name)
    net, sd = _model(cfg, int(g["seed"]), precision)
    x = g.t("x")
    y = _labels(CLASSCOND.index(name) + 7, x.shape[0], cfg.num_classes)
    ref = classcond_forward(sd, cfg, x, g.t("t"), y)
    got = net(x.to(DEV), g.t("t").to(DEV), y.to(DEV)).cpu()
    emax, scale, rms = _report(f"{name} {precision}", got, ref)
    if precision == "fp16":
        assert emax < 0.006 * scale and rms < 0.003
    else:   # bf16 and bf16x2: the bounds of test_gpu_unet.py's bf16 forward.  bf16x2 removes only the weight rounding; on nets this small the
        # bf16 activation storage dominates (measured: mnist bf16x2 2.2 % of scale / 1.4 % rms against bf16's 2.0 % / 1.6 %), so the tighter
        # bf16x2 bound test_gpu_configs.py holds the CIFAR net at B = 256 to does not apply here
        assert emax < 0.04 * scale and rms < 0.02


@pytest.mark.parametrize("name", CLASSCOND)
def test_y_none_is_the_reference(golden, name):
    """A class-conditional model called without labels runs the reference's forward (label_emb unread): the reference fixture."""
    g, cfg = load_case(golden, name)
    net, _ = _model(cfg, int(g["seed"]), "fp32")
    torch.testing.assert_close(net(g.t("x").to(DEV), g.t("t").to(DEV)).cpu(), g.t("y"), rtol=2e-4, atol=5e-5)


def test_zero_label_embedding_is_the_unconditional_model(golden):
    """label_emb = 0: the label path (SiLU after the add, label_emb_linear) computes the unconditional network to fp32 rounding."""
    from image_diffusion.unet import UNetModel, param_shapes

    g, cfg = load_case(golden, "tiny_film_updown_neworder")
    sd = synth_state_dict(param_shapes(cfg), int(g["seed"]))
    sd["label_emb.weight"] = torch.zeros_like(sd["label_emb.weight"])
    net, _ = _model(cfg, 0, "fp32", sd=sd)
    plain = UNetModel(image_size=cfg.image_size, in_channels=cfg.in_channels, model_channels=cfg.model_channels,
                      out_channels=cfg.out_channels, num_res_blocks=cfg.num_res_blocks, attention_resolutions=cfg.attention_resolutions,
                      channel_mult=cfg.channel_mult, num_heads=cfg.num_heads, num_head_channels=cfg.num_head_channels,
                      use_scale_shift_norm=cfg.use_scale_shift_norm, resblock_updown=cfg.resblock_updown,
                      use_new_attention_order=cfg.use_new_attention_order, precision="fp32")
    plain.load_state_dict({k: v for k, v in sd.items() if k != "label_emb.weight"})
    plain.to(DEV)
    x, t = g.t("x").to(DEV), g.t("t").to(DEV)
    y = torch.tensor([4, 0, 2], device=DEV)
    a, b = net(x, t, y).cpu(), plain(x, t).cpu()
    print(f"zero label_emb vs unconditional: max|diff| {(a - b).abs().max().item():.3e}")
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5 * b.abs().max().item())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_batch_independence_of_labels(golden, precision):
    """Image b of a mixed-label batch equals image b of a batch whose labels are all y[b] (same batch size, same launches)."""
    g, cfg = load_case(golden, "mnist")
    net, _ = _model(cfg, int(g["seed"]), precision)
    B = 6
    x = randn(3101, B, 1, 28, 28).to(DEV)
    t = torch.linspace(0.1, 0.9, B).to(DEV)
    y = torch.tensor([7, 0, 3, 9, 3, 1], device=DEV)
    mixed = net(x, t, y).cpu()
    for b in range(B):
        same = net(x, t, torch.full((B,), int(y[b]), device=DEV)).cpu()
        torch.testing.assert_close(mixed[b], same[b], rtol=0, atol=1e-6 * max(1.0, same.abs().max().item()))
    # and the labels matter: different classes give different outputs for the same x, t
    assert (net(x, t, (y + 1) % 10).cpu() - mixed).abs().max() > 1e-3


@pytest.mark.parametrize("n_steps", [50, 200])
def test_cfm_euler_labels_vs_forward_loop(n_steps):
    """engine.cfm_euler(x, t_span, y=) == a loop of forward(t_k, x, y) + euler_step in fp32: Ns = 50 with K = 10 takes the (step, class)
    table (50 * 10 <= 1024 rows), Ns = 200 the per-step fallback.  B = 7 beyond max_batch_override = 3: the slices carry their labels."""
    from mi355.ops import default_ops

    net, _ = _model(MNIST_NB, 3201, "fp32")
    eng = net.engine(DEV)
    B = 7
    x0 = randn(3202 + n_steps, B, 1, 28, 28).to(DEV)
    y = torch.tensor([3, 9, 0, 3, 5, 1, 8], device=DEV)
    ts = torch.linspace(0, 1, n_steps + 1).tolist()
    xl = x0.clone()
    for k in range(n_steps):
        v = eng.forward(xl, ts[k], y=y)
        default_ops.euler_step_(xl, v, ts[k + 1] - ts[k])
    xs = x0.clone()
    eng.cfm_euler(xs, ts, y=y)
    _report(f"cfm_euler labels Ns={n_steps} whole batch", xs.cpu(), xl.cpu())
    torch.testing.assert_close(xs.cpu(), xl.cpu(), rtol=1e-4, atol=1e-4)
    eng.max_batch_override = 3
    try:
        xc = x0.clone()
        eng.cfm_euler(xc, ts, y=y)
    finally:
        eng.max_batch_override = None
    torch.testing.assert_close(xc.cpu(), xl.cpu(), rtol=1e-4, atol=1e-4)
    eng.check()


def test_notebook_mnist_dopri5_vs_restatement():
    """conditional_mnist.ipynb: torchcfm's UNetModel (ClassCondUNetModelWrapper here)(dim=(1, 28, 28), num_channels=32, num_res_blocks=1, num_classes=10, class_cond=True)
    sampled with odeint(lambda t, x: model.forward(t, x, labels), x0, [0, 1], dopri5), B = 100, labels arange(10).repeat(10), against
    oracle.cfm_ref.dopri5 over the restated vector field ('parity unpinned': torchdiffeq is not vendored)."""
    from image_diffusion.unet import param_shapes
    from mi355.ode import odeint_dopri5
    from torchcfm_compat import ClassCondUNetModelWrapper

    m = ClassCondUNetModelWrapper(dim=(1, 28, 28), num_channels=32, num_res_blocks=1, num_classes=10, class_cond=True, precision="fp32")
    sd = synth_state_dict(param_shapes(m), 3301)
    assert list(sd) == list(param_shapes(MNIST_NB))
    m.load_state_dict(sd)
    m.to(DEV)
    B = 100
    y = torch.arange(10).repeat(10)
    x0 = randn(3302, B, 1, 28, 28)
    got, nfe = odeint_dopri5(lambda t, x: m.forward(t, x, y.to(DEV)), x0.to(DEV), 0.0, 1.0, 1e-4, 1e-4)
    f = lambda t, x: classcond_forward(sd, MNIST_NB, x, t.reshape(1).repeat(B), y)
    ref, nfe_ref = cfm_ref.dopri5(f, x0, 0.0, 1.0, 1e-4, 1e-4)
    _report(f"notebook dopri5 (nfe {nfe} vs {nfe_ref})", got.cpu(), ref)
    torch.testing.assert_close(got.cpu(), ref, rtol=3e-3, atol=3e-3)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_vjp_with_labels_vs_autograd(golden, precision):
    """The differentiable engine's data gradient through a labelled forward against torch.autograd through the restatement."""
    g, cfg = load_case(golden, "tiny_film_updown_neworder")
    net, sd = _model(cfg, int(g["seed"]), precision)
    B = 4
    x = randn(3401, B, cfg.in_channels, cfg.image_size, cfg.image_size)
    t = torch.tensor([0.05, 0.3, 0.62, 0.97])
    y = torch.tensor([4, 1, 1, 0])
    cot = randn(3402, B, cfg.out_channels, cfg.image_size, cfg.image_size)
    xr = x.clone().requires_grad_()
    (ref,) = torch.autograd.grad((classcond_forward(sd, cfg, xr, t, y) * cot).sum(), xr)
    eng = net.engine(DEV, differentiable=True)
    eng.forward(x.to(DEV), t.to(DEV), y=y.to(DEV))
    got = eng.vjp(cot.to(DEV)).cpu()
    if precision == "fp32":
        torch.testing.assert_close(got, ref, rtol=2e-3, atol=5e-4 * float(ref.abs().max()))
    else:   # per image, the bounds test_gpu_guidance.py holds the bf16 backward of its small synthetic nets to
        dims = (1, 2, 3)
        rms = (got - ref).pow(2).mean(dim=dims).sqrt() / ref.pow(2).mean(dim=dims).sqrt()
        mx = (got - ref).abs().amax(dim=dims) / ref.abs().amax(dim=dims)
        print(f"bf16 vjp with labels: worst relative rms {float(rms.max()):.3e}, worst max|err|/max|ref| {float(mx.max()):.3e}")
        assert torch.isfinite(got).all() and float(rms.max()) < 0.07 and float(mx.max()) < 0.075


def test_out_of_range_label_raises_and_valid_images_hold(golden):
    """A label outside [0, K) reads nothing outside label_emb: the engine reports it (MI355_ERR_ARG naming the labels) at check() or the
    next call, and the other images of the batch are still right.  Both the forward and the sampler's gather path."""
    from mi355._lib import MI355BackendError

    g, cfg = load_case(golden, "tiny")
    net, sd = _model(cfg, int(g["seed"]), "fp32")
    eng = net.engine(DEV)
    x, t = g.t("x"), g.t("t")
    y = torch.tensor([2, cfg.num_classes, 0])
    out = eng.forward(x.to(DEV), t.to(DEV), y=y.to(DEV)).cpu()
    torch.cuda.synchronize()
    with pytest.raises(MI355BackendError, match="label"):
        eng.forward(x.to(DEV), t.to(DEV), y=torch.tensor([0, 1, 2], device=DEV))   # the next call reports it ...
    with pytest.raises(MI355BackendError, match="label"):
        eng.check()                                                                   # ... until check() clears it
    ok = [0, 2]
    ref = classcond_forward(sd, cfg, x[ok], t[ok], y[ok])
    torch.testing.assert_close(out[ok], ref, rtol=2e-4, atol=5e-5)
    eng.check()
    # (the sampler's second step may already see the flag on entry: then cfm_euler itself raises, and the flag stays until a check())
    with pytest.raises(MI355BackendError, match="label"):
        eng.cfm_euler(x.to(DEV).clone(), [0.0, 0.5, 1.0], y=torch.tensor([1, -1, 3], device=DEV))
        torch.cuda.synchronize()
        eng.check()
    torch.cuda.synchronize()
    try:
        eng.check()
    except MI355BackendError:
        pass
    eng.check()


def test_table_step_adds_one_launch():
    """One Euler step on the (step, class) table costs the unconditional step's launches + 1 (the row gather)."""
    net, _ = _model(MNIST_NB, 3501, "bf16")
    eng = net.engine(DEV)
    x = randn(3502, 4, 1, 28, 28).to(DEV)
    eng.cfm_euler(x.clone(), [0.0, 0.5])
    n_uncond = eng.stats(4)["launches"]
    eng.cfm_euler(x.clone(), [0.0, 0.5], y=torch.tensor([0, 9, 4, 4], device=DEV))
    n_label = eng.stats(4)["launches"]
    eng.forward(x, 0.5, y=torch.tensor([0, 9, 4, 4], device=DEV))
    n_single = eng.stats(4)["launches"]
    torch.cuda.synchronize()
    eng.check()
    print(f"launches per step: unconditional {n_uncond}, table path {n_label}, single labelled forward {n_single}")
    assert n_label == n_uncond + 1
