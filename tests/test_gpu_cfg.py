"""GPU: classifier-free guidance on the HIP path - the guided update kernels op by op (bit-exact against the existing ops applied to a
torch-computed guided field), the fused samplers mi355_cfm_cfg_sample / mi355_ddpm_cfg_sample against host loops built from existing
pieces (forward(conditional), forward(unconditional), the torch expression u + w * (c - u), the existing step ops), the guided single
forward against the CPU restatement, the library's refusals and its workspace rule.

Tolerance of the sampler comparisons: the fused call and the host loop share every kernel and differ by batch size (summation order)
alone; the unguided comparison test_gpu_classcond.test_cfm_euler_labels_vs_forward_loop holds rtol = atol = 1e-4, and a guided field
carries (1 + 2|w|) times the per-evaluation difference: 1e-4 * (1 + 2|w|).

Observed on an MI355X (fp32): see DESIGN.md section 8.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mi355.synth import randn, synth_state_dict
from tests.test_classcond_cpu import CLASSCOND, ClassCondConfig, classcond_forward, load_case
from tests.test_gpu_classcond import MNIST_NB, _model
from tests.test_oracle_golden import cfg_from_json

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NULL = 9   # MNIST_NB has 10 classes: 0..8 are real, the last one is the null token


def _bound(w):
    b = 1e-4 * (1 + 2 * abs(float(w)))
    return dict(rtol=b, atol=b)


def _report(tag, got, ref):
    d = (got - ref).abs().max().item()
    print(f"{tag}: max|diff| {d:.3e} (scale {ref.abs().max().item():.3f})")
    return d


def _mix(c, u, w):
    """u + w * (c - u) in eager torch: the difference, the product and the sum each rounded to fp32.  w: a float or a [B] tensor."""
    if isinstance(w, torch.Tensor):
        w = w.reshape(-1, *([1] * (c.dim() - 1)))
    d = c - u
    p = d * w
    return u + p


# ---- op level ---------------------------------------------------------------------------------------------------------------------

SHAPES = [(3, (1, 5, 7)), (4, (3, 8, 8))]   # n = 105: half base not 16-byte aligned, ragged last vector; n = 768: the all-aligned vector path


def _w_of(per_image, B):
    return torch.tensor([0.5 + 0.75 * b for b in range(B)], device=DEV) if per_image else 1.75


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("nk", [1, 2, 3, 4])
@pytest.mark.parametrize("B,img", SHAPES)
def test_cfg_stage_bit_exact(B, img, nk, per_image):
    from mi355.ops import default_ops as ops

    w = _w_of(per_image, B)
    ks = [randn(4100 + 10 * nk + j, 2 * B, *img).to(DEV) for j in range(nk)]
    coeffs = [0.3, -0.125, 0.7, 1.1][:nk]
    gs = [_mix(k[:B], k[B:], w).contiguous() for k in ks]
    y0 = randn(4190, B, *img).to(DEV)
    for with_y0, dup, extras in [(True, False, False), (True, True, True), (False, False, True), (False, True, False)]:
        base = y0 if with_y0 else torch.zeros_like(y0)
        exp, exp_copy, exp_u8 = torch.empty_like(y0), torch.empty_like(y0), torch.empty(y0.shape, dtype=torch.uint8, device=DEV)
        ops.rk_stage(exp, base, gs, coeffs, copy_out=exp_copy, u8_out=exp_u8)
        out = torch.full((2 * B if dup else B, *img), float("nan"), device=DEV)
        cp = torch.full_like(y0, float("nan")) if extras else None
        u8 = torch.zeros(y0.shape, dtype=torch.uint8, device=DEV) if extras else None
        ops.cfg_stage(out, y0 if with_y0 else None, ks, coeffs, w, dup=dup, copy_out=cp, u8_out=u8)
        assert torch.equal(out[:B], exp), (with_y0, dup)
        if dup:
            assert torch.equal(out[B:], exp)
        if extras:
            assert torch.equal(cp, exp) and torch.equal(u8, exp_u8)
    # in place on a duplicated state, as the sampler's update runs
    x2 = torch.cat((y0, y0))
    ops.rk_stage(exp, y0, gs, coeffs)
    ops.cfg_stage(x2, x2, ks, coeffs, w, dup=True)
    assert torch.equal(x2[:B], exp) and torch.equal(x2[B:], exp)
    assert (exp - y0).abs().max() > 0.1


@pytest.mark.parametrize("per_image", [False, True])
def test_cfg_stage_odd_storage_offset_and_empty(per_image):
    """Views one float into their storage (4-byte aligned only: the scalar path on a size the vector path would take) and n = 0."""
    from mi355.ops import default_ops as ops

    B, img = 4, (3, 8, 8)
    n = B * 3 * 64
    w = _w_of(per_image, B)
    k = torch.empty(2 * n + 1, device=DEV)[1:].view(2 * B, *img)
    k.copy_(randn(4201, 2 * B, *img))
    y0 = torch.empty(n + 1, device=DEV)[1:].view(B, *img)
    y0.copy_(randn(4202, B, *img))
    out = torch.empty(2 * n + 1, device=DEV)[1:].view(2 * B, *img)
    assert k.data_ptr() % 16 == 4 and k.is_contiguous()
    g = _mix(k[:B], k[B:], w).contiguous()
    exp = torch.empty(B, *img, device=DEV)
    ops.rk_stage(exp, y0.clone(), [g], [0.4])
    ops.cfg_stage(out, y0, [k], [0.4], w, dup=True)
    assert torch.equal(out[:B], exp) and torch.equal(out[B:], exp)
    # cfg_combine: the guided field itself
    assert torch.equal(ops.cfg_combine(k, w), g + 0.0)
    e = torch.empty(0, 3, 8, 8, device=DEV)
    ops.cfg_stage(e, None, [e], [1.0], 2.0)
    ops.ddim_cfg_step_(e, e, 2.0, 1.0, 1.0, 0.5)
    torch.cuda.synchronize()


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("B,img", SHAPES)
def test_ddpm_and_ddim_cfg_step_bit_exact(B, img, per_image):
    from mi355._lib import MI355BackendError
    from mi355.ops import default_ops as ops

    w = _w_of(per_image, B)
    x = randn(4301, B, *img).to(DEV)
    eps2 = randn(4302, 2 * B, *img).to(DEV)
    z = randn(4303, B, *img).to(DEV)
    eg = _mix(eps2[:B], eps2[B:], w).contiguous()
    co = (1.8, 1.5, 0.3, 0.65, 0.2)
    for zz, ph in ((z, None), (None, (77, 8)), (None, None)):
        exp = ops.ddpm_step_(x.clone(), eg, zz, *co, philox=ph)
        x2 = torch.cat((x, x + 5.0))   # the second half is never read
        ops.ddpm_cfg_step_(x2, eps2, zz, w, *co, philox=ph)
        assert torch.equal(x2[:B], exp) and torch.equal(x2[B:], exp), (zz is None, ph)
    exp = ops.ddim_step_(x.clone(), eg, 1.8, 1.5, 0.6)
    x2 = torch.cat((x, x + 5.0))
    ops.ddim_cfg_step_(x2, eps2, w, 1.8, 1.5, 0.6)
    assert torch.equal(x2[:B], exp) and torch.equal(x2[B:], exp)
    assert (exp - x).abs().max() > 0.05
    with pytest.raises(MI355BackendError, match="multiple of 4"):
        ops.ddpm_cfg_step_(torch.cat((x, x)), eps2, None, w, *co, philox=(77, 6))


# ---- CFM sampler ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mnist_eng():
    net, _ = _model(MNIST_NB, 5101, "fp32")
    return net.engine(DEV)


Y7 = [3, 0, 8, 3, 5, 1, 8]


def _guided(eng, x, t, y, w, null=NULL):
    vc = eng.forward(x, t, y=y)
    vu = eng.forward(x, t, y=torch.full_like(y, null))
    return _mix(vc, vu, w)


_HOST = {}


def _host_loop(eng, method, n_steps, w_key, x0, y, w):
    """The loop a user writes today, once per (method, steps, scale): all states."""
    key = (method, n_steps, w_key)
    if key not in _HOST:
        from mi355.ode import FixedStepRK
        from mi355.ops import default_ops

        ts = torch.linspace(0, 1, n_steps + 1).tolist()
        if method == "euler":
            xl, states = x0.clone(), [x0.clone()]
            for k in range(n_steps):
                default_ops.euler_step_(xl, _guided(eng, xl, ts[k], y, w).contiguous(), ts[k + 1] - ts[k])
                states.append(xl.clone())
        else:
            sol = FixedStepRK(lambda t, s: [_guided(eng, s[0], float(t), y, w)], method)
            states = [x0.clone()] + [s[0].clone() for s in sol.integrate_times([x0.clone()], ts)]
        _HOST[key] = torch.stack(states).cpu()
    return _HOST[key]


@pytest.mark.parametrize("method,n_steps", [("euler", 50), ("euler", 200), ("rk4", 20), ("rk4", 50), ("rk4", 200)])
def test_cfm_cfg_vs_host_loop(mnist_eng, method, n_steps):
    """K = 10: Euler at 50 steps and rk4 at 20 take the (step, class) table (500 / 800 rows), the others per-evaluation rows.  B = 7, w = 2;
    the 50-step cases once more through max_batch_override = 3 (guided slices of one image)."""
    eng = mnist_eng
    w = 2.0
    x0 = randn(5200 + n_steps, 7, 1, 28, 28).to(DEV)
    y = torch.tensor(Y7, device=DEV)
    ts = torch.linspace(0, 1, n_steps + 1).tolist()
    ref = _host_loop(eng, method, n_steps, "w2", x0, y, w)
    run = (lambda x, **kw: eng.cfm_euler(x, ts, y=y, guidance_scale=w, null_label=NULL, **kw)) if method == "euler" else \
        (lambda x, **kw: eng.cfm_rk(x, ts, method, y=y, guidance_scale=w, null_label=NULL, **kw))
    xs = x0.clone()
    _, traj, u8 = run(xs, keep_traj=True, want_u8=True)
    _report(f"cfm cfg {method} Ns={n_steps} w=2 whole batch", xs.cpu(), ref[-1])
    torch.testing.assert_close(xs.cpu(), ref[-1], **_bound(w))
    # trajectory slots and image bytes: the states of the host loop; the last slot and the bytes are the final state's own
    torch.testing.assert_close(traj.cpu(), ref, **_bound(w))
    assert torch.equal(traj[0], x0) and torch.equal(traj[-1], xs)
    from mi355.ops import default_ops

    assert torch.equal(u8, default_ops.quantize_u8(xs))
    ref_u8 = (ref[-1] * 127.5 + 128).clip(0, 255).to(torch.uint8)
    assert (u8.cpu().int() - ref_u8.int()).abs().max() <= 1
    if n_steps == 50:
        eng.max_batch_override = 3
        try:
            xc = x0.clone()
            _, tc, uc = run(xc, keep_traj=True, want_u8=True)
        finally:
            eng.max_batch_override = None
        _report(f"cfm cfg {method} Ns={n_steps} w=2 slices", xc.cpu(), ref[-1])
        torch.testing.assert_close(xc.cpu(), ref[-1], **_bound(w))
        assert torch.equal(tc[-1], xc) and torch.equal(uc, default_ops.quantize_u8(xc))
    torch.cuda.synchronize()
    eng.check()


def test_cfm_cfg_per_image_scale(mnist_eng):
    eng = mnist_eng
    wt = torch.tensor([0.0, 1.0, 2.0, 3.0, -0.5, 1.5, 2.5], device=DEV)
    x0 = randn(5301, 7, 1, 28, 28).to(DEV)
    y = torch.tensor(Y7, device=DEV)
    ts = torch.linspace(0, 1, 51).tolist()
    ref = _host_loop(eng, "euler", 50, "per_image", x0, y, wt)[-1]
    for override in (None, 3):
        eng.max_batch_override = override
        try:
            xs = x0.clone()
            eng.cfm_euler(xs, ts, y=y, guidance_scale=wt, null_label=NULL)
        finally:
            eng.max_batch_override = None
        _report(f"cfm cfg euler per-image w, max_batch_override {override}", xs.cpu(), ref)
        torch.testing.assert_close(xs.cpu(), ref, **_bound(3.0))
    # the scales reach their own images: image 0 (w = 0) is the unconditional sample, image 1 (w = 1) the conditional one
    xu, xc = x0.clone(), x0.clone()
    eng.cfm_euler(xu, ts, y=torch.full_like(y, NULL))
    eng.cfm_euler(xc, ts, y=y)
    torch.testing.assert_close(xs[0].cpu(), xu[0].cpu(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(xs[1].cpu(), xc[1].cpu(), **_bound(1.0))
    eng.check()


def test_cfm_cfg_identities(mnist_eng):
    """w = 0 is the unconditional sampler (unguided bound), w = 1 the conditional one (guided bound), and w = 3 is far from w = 1: the
    floor is ten times the w = 3 bound (test_gpu_classcond holds a label change to > 1e-3 in ONE evaluation; here 50 steps integrate twice
    the conditional-unconditional difference)."""
    eng = mnist_eng
    x0 = randn(5401, 7, 1, 28, 28).to(DEV)
    y = torch.tensor(Y7, device=DEV)
    ts = torch.linspace(0, 1, 51).tolist()
    out = {}
    for w in (0.0, 1.0, 3.0):
        out[w] = x0.clone()
        eng.cfm_euler(out[w], ts, y=y, guidance_scale=w, null_label=NULL)
    xu, xc = x0.clone(), x0.clone()
    eng.cfm_euler(xu, ts, y=torch.full_like(y, NULL))
    eng.cfm_euler(xc, ts, y=y)
    _report("w = 0 vs unconditional", out[0.0].cpu(), xu.cpu())
    _report("w = 1 vs conditional", out[1.0].cpu(), xc.cpu())
    far = _report("w = 3 vs w = 1", out[3.0].cpu(), out[1.0].cpu())
    torch.testing.assert_close(out[0.0].cpu(), xu.cpu(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out[1.0].cpu(), xc.cpu(), **_bound(1.0))
    assert far > 10 * _bound(3.0)["atol"]
    eng.check()


def test_guided_single_time_is_a_no_op(mnist_eng):
    """n_t == 1 on the guided entry point, as test_gpu_rk.test_single_time_is_a_no_op on the plain one: no step; traj[0] and the uint8
    output are still written."""
    from mi355.ops import default_ops

    x0 = randn(5402, 3, 1, 28, 28).to(DEV)
    x = x0.clone()
    _, traj, u8 = mnist_eng.cfm_rk(x, [0.3], "rk4", y=torch.tensor([3, 0, 8], device=DEV), guidance_scale=2.0, null_label=NULL,
                                   keep_traj=True, want_u8=True)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and traj.shape[0] == 1 and torch.equal(traj[0], x0) and torch.equal(u8, default_ops.quantize_u8(x0))
    mnist_eng.check()


def test_guided_step_launch_counts():
    """stats() after a guided call: every launch of the last step = `stages` evaluations (each a labelled table-path evaluation at 2B)
    plus `stages` stage launches; nothing else (no per-step copy)."""
    net, _ = _model(MNIST_NB, 5501, "bf16")
    eng = net.engine(DEV)
    x = randn(5502, 4, 1, 28, 28).to(DEV)
    y = torch.tensor([0, 8, 4, 4], device=DEV)
    eng.cfm_euler(torch.cat((x, x)), [0.0, 0.5], y=torch.cat((y, y)))
    n_eval = eng.stats(8)["launches"]   # one labelled evaluation at batch 8 on the table path (the Euler update is not counted)
    eng.cfm_euler(x.clone(), [0.0, 0.5], y=y, guidance_scale=2.0, null_label=NULL)
    n_euler = eng.stats(8)["launches"]
    eng.cfm_rk(x.clone(), [0.0, 0.5], "rk4", y=y, guidance_scale=2.0, null_label=NULL)
    n_rk4 = eng.stats(8)["launches"]
    torch.cuda.synchronize()
    eng.check()
    print(f"launches: one labelled evaluation at 2B {n_eval}, guided Euler step {n_euler}, guided rk4 step {n_rk4}")
    assert n_euler == n_eval + 1
    assert n_rk4 == 4 * n_eval + 4


@pytest.mark.parametrize("name", CLASSCOND)
def test_forward_guided_vs_restatement(golden, name):
    g, cfg = load_case(golden, name)
    net, sd = _model(cfg, int(g["seed"]), "fp32")
    x, t = g.t("x"), g.t("t")
    B, K = x.shape[0], cfg.num_classes
    y = torch.tensor([(2 * b + 1) % (K - 1) for b in range(B)])
    w = 2.0
    vc = classcond_forward(sd, cfg, x, t, y)
    vu = classcond_forward(sd, cfg, x, t, torch.full_like(y, K - 1))
    ref = vu + w * (vc - vu)
    eng = net.engine(DEV)
    got = eng.forward(x.to(DEV), t.to(DEV), y=y.to(DEV), guidance_scale=w).cpu()       # null_label defaults to the last class
    _report(f"guided forward {name}", got, ref)
    torch.testing.assert_close(got, ref, rtol=2e-4 * 5, atol=5e-5 * 5)
    eng.max_batch_override = 2   # slices of one image
    try:
        got_s = eng.forward(x.to(DEV), t.to(DEV), y=y.to(DEV), guidance_scale=torch.full((B,), w, device=DEV), null_label=K - 1).cpu()
    finally:
        eng.max_batch_override = None
    torch.testing.assert_close(got_s, ref, rtol=2e-4 * 5, atol=5e-5 * 5)
    assert (vc - vu).abs().max() > 1e-3
    eng.check()


def test_forward_guided_bf16(golden):
    g, cfg = load_case(golden, "mnist")
    net, sd = _model(cfg, int(g["seed"]), "bf16")
    x, t = g.t("x"), g.t("t")
    y = torch.tensor([1, 4, 7])
    w = 2.0
    vu = classcond_forward(sd, cfg, x, t, torch.full_like(y, 9))
    ref = vu + w * (classcond_forward(sd, cfg, x, t, y) - vu)
    got = net.engine(DEV).forward(x.to(DEV), t.to(DEV), y=y.to(DEV), guidance_scale=w, null_label=9).cpu()
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    rms = ((got - ref) ** 2).mean().sqrt().item() / ref.pow(2).mean().sqrt().item()
    print(f"guided forward bf16: max|err| {err:.3e} (scale {scale:.3f}), rel rms {rms:.3e}")
    assert err < 0.04 * scale * 5 and rms < 0.02 * 5


def test_neural_ode_guided_vector_field(mnist_eng):
    """NeuralODE(GuidedVectorField) sends a fixed-step solve to the library in one call; dopri5 drives the guided forward."""
    from mi355.ode import odeint_dopri5
    from torchcfm_compat import ClassCondUNetModelWrapper, GuidedVectorField, NeuralODE

    m = ClassCondUNetModelWrapper(dim=(1, 28, 28), num_channels=32, num_res_blocks=1, num_classes=10, class_cond=True, precision="fp32")
    from image_diffusion.unet import param_shapes

    m.load_state_dict(synth_state_dict(param_shapes(m), 5101))
    m.to(DEV)
    x0 = randn(5200 + 50, 7, 1, 28, 28).to(DEV)
    y = torch.tensor(Y7, device=DEV)
    ref = _host_loop(mnist_eng, "euler", 50, "w2", x0, y, 2.0)
    traj = NeuralODE(GuidedVectorField(m, y=y, guidance_scale=2.0, null_label=NULL), solver="euler").trajectory(x0, torch.linspace(0, 1, 51))
    torch.testing.assert_close(traj.cpu(), ref, **_bound(2.0))
    a, nfe = odeint_dopri5(lambda t, x: m(t, x, y[:2], guidance_scale=2.0, null_label=NULL), x0[:2].clone(), 0.0, 1.0, 1e-3, 1e-3)
    b, _ = odeint_dopri5(lambda t, x: _guided(m.engine(DEV), x, float(t), y[:2], 2.0), x0[:2].clone(), 0.0, 1.0, 1e-3, 1e-3)
    _report(f"guided dopri5 (nfe {nfe}) vs two-forward field", a.cpu(), b.cpu())
    torch.testing.assert_close(a.cpu(), b.cpu(), rtol=3e-3, atol=3e-3)   # the adaptive solver's own tolerance class (test_gpu_classcond)


# ---- DDPM sampler -----------------------------------------------------------------------------------------------------------------

NS = 25


@pytest.fixture(scope="module")
def in6(golden):
    from tests.test_gpu_unet import build

    g = golden("unet_tiny_in6")
    net, _ = build(cfg_from_json(g.json("config")), int(g["seed"]), "fp32")
    return net


def _ddpm_inputs(C=3, B=3, S=16):
    xT = randn(5601, B, C, S, S).to(DEV)
    cond = (randn(5602, B, C, S, S) * 0.5).clamp(-1, 1)
    cond[:, :, 4:10, 5:11] = -2.0
    noise = torch.stack([randn(5610 + j, B, C, S, S) for j in range(2 * NS)]).to(DEV)
    return xT, cond.to(DEV), noise


def _ddpm_host(eng, xT, cond, w, noise, n_corrector=0, ddim=False, delta=0.1, y=None, null=None, none=-2.0):
    """forward(cond), forward(none), the torch expression, the existing step ops; draws in mi355_ddpm_sample's order."""
    from image_diffusion.sde_diffusion import DDPM
    from mi355.ops import default_ops as ops

    ddpm = DDPM(NS)
    T = ddpm.host_tables()
    xi = xT.clone()
    nonec = torch.full_like(cond, none)
    yn = torch.full_like(y, null) if y is not None else None
    draw = 0
    for i in reversed(range(NS)):
        t = float(np.float32(i) / np.float32(NS))
        ec = eng.forward(xi, t, cond=cond, y=y)
        eu = eng.forward(xi, t, cond=nonec, y=yn)
        eps = _mix(ec, eu, w).contiguous()
        cr, cm = float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i])
        if ddim:
            ops.ddim_step_(xi, eps, cr, cm, float(T["alphas_cumprod_prev"][i]))
            continue
        z = None
        if i > 0:
            z, draw = noise[draw], draw + 1
        sigma = float(np.exp(np.float32(0.5) * np.float32(float(T["posterior_log_variance_clipped"][i]))))
        ops.ddpm_step_(xi, eps, z, cr, cm, float(T["posterior_mean_coef1"][i]), float(T["posterior_mean_coef2"][i]), sigma)
        for _ in range(n_corrector):
            e = eng.forward(xi, t, cond=nonec, y=yn)
            ops.corrector_step_(xi, e, noise[draw], cr, cm, float(T["recip_sqrt_m1_alphas_cumprod"][i]), (ddpm.tmax - ddpm.tmin) / NS, delta)
            draw += 1
    return ops.clip_(xi), T, ddpm


@pytest.mark.parametrize("case", ["amortized", "amortized_corr1", "ddim"])
def test_ddpm_cfg_vs_host_loop(in6, case):
    from mi355 import _lib

    eng = in6.engine(DEV)
    xT, cond, noise = _ddpm_inputs()
    w = 2.0
    nc, ddim = int(case == "amortized_corr1"), case == "ddim"
    ref, T, ddpm = _ddpm_host(eng, xT, cond, w, noise, n_corrector=nc, ddim=ddim)
    got = eng.ddpm_sample(xT.clone(), T, mode=_lib.DDIM if ddim else _lib.DDPM_AMORTIZED, cond=cond, noise=None if ddim else noise,
                          n_corrector=nc, delta=0.1, tmin=ddpm.tmin, tmax=ddpm.tmax, guidance_scale=w)
    _report(f"ddpm cfg {case} w=2", got.cpu(), ref.cpu())
    torch.testing.assert_close(got.cpu(), ref.cpu(), **_bound(w))
    eng.max_batch_override = 2   # slices of one image, each with its rows of the injected draws
    try:
        got_s = eng.ddpm_sample(xT.clone(), T, mode=_lib.DDIM if ddim else _lib.DDPM_AMORTIZED, cond=cond, noise=None if ddim else noise,
                                n_corrector=nc, delta=0.1, tmin=ddpm.tmin, tmax=ddpm.tmax, guidance_scale=torch.full((3,), w, device=DEV))
    finally:
        eng.max_batch_override = None
    torch.testing.assert_close(got_s.cpu(), ref.cpu(), **_bound(w))
    eng.check()


def test_cfg_conditioning_fast_and_generic_paths(in6):
    from image_diffusion import sampling
    from image_diffusion.conditioning import ClassifierFreeGuidance
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM

    ddpm = DDPM(NS)
    lik = InPainting(patch_size=6, pad_value=-2)
    xT, cond, noise = _ddpm_inputs()
    cfg = ClassifierFreeGuidance(0.9, 1, 0.1, 2.0)
    outs = []
    for eps_model in (sampling.make_eps_model(in6, ddpm), lambda xi, i: in6(xi, 1.0 * i / ddpm.Ns)):
        with sampling.injected_noise(list(noise)):
            outs.append(sampling.get_conditional_sample_fn(eps_model, ddpm, cfg, lik)(xT, cond).cpu())
    ref, _, _ = _ddpm_host(in6.engine(DEV), xT, cond, 2.0, noise, n_corrector=1)
    _report("ClassifierFreeGuidance fast vs generic", outs[0], outs[1])
    torch.testing.assert_close(outs[0], outs[1], **_bound(2.0))
    torch.testing.assert_close(outs[0], ref.cpu(), **_bound(2.0))
    with sampling.injected_noise(list(noise)):
        d = [sampling.get_ddim_sample_fn(e, ddpm, lik, guidance_scale=2.0)(xT, cond).cpu()
             for e in (sampling.make_eps_model(in6, ddpm), lambda xi, i: in6(xi, 1.0 * i / ddpm.Ns))]
    torch.testing.assert_close(d[0], d[1], **_bound(2.0))


def test_ddpm_cfg_w1_philox_is_the_unguided_sampler(in6):
    from mi355 import _lib
    from image_diffusion.sde_diffusion import DDPM

    eng = in6.engine(DEV)
    ddpm = DDPM(NS)
    T = ddpm.host_tables()
    xT, cond, _ = _ddpm_inputs()
    kw = dict(mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1, delta=0.1, tmin=ddpm.tmin, tmax=ddpm.tmax, seed=1234)
    a = eng.ddpm_sample(xT.clone(), T, **kw)
    b = eng.ddpm_sample(xT.clone(), T, guidance_scale=1.0, **kw)
    c = eng.ddpm_sample(xT.clone(), T, guidance_scale=1.0, **dict(kw, seed=1235))
    _report("ddpm cfg w=1 (Philox) vs unguided", b.cpu(), a.cpu())
    torch.testing.assert_close(b.cpu(), a.cpu(), **_bound(1.0))
    assert (c - b).abs().max() > 1e-2   # the seed is used
    eng.check()


def test_ddpm_cfg_labels_and_condition():
    """A class-conditional 2C-input net: labels and a condition guided together in one call."""
    from mi355 import _lib

    cfg = ClassCondConfig(16, 2, 32, 1, 1, (2,), channel_mult=(1, 2), num_heads=2, num_classes=4)
    net, _ = _model(cfg, 5701, "fp32")
    eng = net.engine(DEV)
    xT, cond, noise = _ddpm_inputs(C=1)
    y = torch.tensor([2, 0, 1], device=DEV)
    w = 2.0
    ref, T, ddpm = _ddpm_host(eng, xT, cond, w, noise, y=y, null=3)
    got = eng.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_AMORTIZED, cond=cond, noise=noise, tmin=ddpm.tmin, tmax=ddpm.tmax,
                          guidance_scale=w, y=y, null_label=3)
    _report("ddpm cfg labels + condition w=2", got.cpu(), ref.cpu())
    torch.testing.assert_close(got.cpu(), ref.cpu(), **_bound(w))
    other = eng.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_AMORTIZED, cond=cond, noise=noise, tmin=ddpm.tmin, tmax=ddpm.tmax,
                            guidance_scale=w, y=(y + 1) % 3, null_label=3)
    assert (other - got).abs().max() > 1e-3   # the labels matter
    eng.check()


# ---- refusals and the workspace rule (host-only checks of the library; they need a handle, hence a device) -----------------------------

def _al(v):
    return (v + 255) // 256 * 256


def test_workspace_rule_and_refusals(in6, mnist_eng):
    from mi355 import _lib
    from mi355._lib import MI355BackendError, check
    from image_diffusion.sde_diffusion import DDPM

    L = _lib.lib()
    for eng, cond_c in ((in6.engine(DEV), 3), (mnist_eng, 0)):
        B = 5
        base = _al(L.mi355_unet_workspace_bytes(eng.handle, 2 * B))
        st = _al(2 * B * eng.out_channels * eng.image_size ** 2 * 4)
        tail = st + (_al(2 * B * cond_c * eng.image_size ** 2 * 4) if cond_c else 0) + (_al(2 * B * 4) if eng.num_classes else 0)
        for stages in (1, 2, 4):
            assert L.mi355_cfg_workspace_bytes(eng.handle, B, stages) == base + tail + (stages + (stages > 1)) * st
        assert L.mi355_ddpm_cfg_workspace_bytes(eng.handle, B) == base + tail
        assert L.mi355_cfg_workspace_bytes(eng.handle, B, 0) < 0 and L.mi355_cfg_workspace_bytes(eng.handle, B, 5) < 0

    eng = mnist_eng
    B = 2
    x = randn(5801, B, 1, 28, 28).to(DEV)
    y = torch.tensor([1, 2], device=DEV, dtype=torch.int32)
    need = L.mi355_cfg_workspace_bytes(eng.handle, B, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ts = (C.c_float * 2)(0.0, 1.0)
    one, zero = (C.c_float * 16)(*([1.0] * 16)), (C.c_float * 16)()
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731

    def cfm(labels=y, null=9, stages=1, wsb=need, cond=None, cc=0, b=one):
        return L.mi355_cfm_cfg_sample(eng.handle, vp(x), 1, vp(cond), cc, -2.0, vp(labels), null, 2.0, None, ts, 2, stages, zero, b, zero, None, None,
                                      B, vp(ws), wsb, None)

    before = x.clone()
    for kw, msg in ((dict(null=10), "null_label"), (dict(null=-1), "null_label"), (dict(labels=None), "nothing to guide"),
                    (dict(stages=0), "1 to 4"), (dict(stages=5), "1 to 4"), (dict(wsb=need - 256), "workspace too small"),
                    (dict(b=zero), "all zero")):
        with pytest.raises(MI355BackendError, match=msg):
            check(cfm(**kw), "mi355_cfm_cfg_sample")
    assert cfm(null=10) == -1 and cfm(labels=None) == -1 and cfm(wsb=need - 256) == -2
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    eng.check()   # an out-of-range null_label never reached the device error word

    e6 = in6.engine(DEV)
    xT, cond, noise = _ddpm_inputs()
    T = DDPM(NS).host_tables()
    with pytest.raises(MI355BackendError, match="without num_classes"):
        e6._ddpm_cfg_call(xT.clone(), T, _lib.DDPM_AMORTIZED, cond, torch.zeros(3, dtype=torch.int32, device=DEV), 0, 2.0, None, noise,
                          dict(n_corrector=0, delta=0.1, tmin=1e-5, tmax=1.0, none_value=-2.0, seed=0))
    for mode in (_lib.DDPM_PRIOR, _lib.DDPM_REPLACEMENT):
        with pytest.raises(MI355BackendError, match="prior and replacement"):
            e6._ddpm_cfg_call(xT.clone(), T, mode, cond, None, 0, 2.0, None, noise,
                              dict(n_corrector=0, delta=0.1, tmin=1e-5, tmax=1.0, none_value=-2.0, seed=0))
    with pytest.raises(MI355BackendError, match="nothing to guide"):
        e6._ddpm_cfg_call(xT.clone(), T, _lib.DDPM_AMORTIZED, None, None, 0, 2.0, None, noise,
                          dict(n_corrector=0, delta=0.1, tmin=1e-5, tmax=1.0, none_value=-2.0, seed=0))
    with pytest.raises(MI355BackendError, match="per-image"):   # n = 10 is no whole number of 3-element images
        check(L.mi355_cfg_stage(vp(x), None, (C.c_void_p * 4)(x.data_ptr()), one, 1, 10, 2.0, vp(x), 3, 0, None, None, None))
    torch.cuda.synchronize()
    e6.check()
