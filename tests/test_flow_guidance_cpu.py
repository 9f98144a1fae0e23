"""CPU: the host side of the training-free flow in-painting / super-resolution samplers - the new symbols, the CPU restatement the GPU
tests compare against (tests/flow_guidance_ref.py: its gather-form adjoint of the bilinear reduction against torch.autograd in fp64, and a
first-order descent check of its guidance gradient), the LowResolution likelihood, the two conditioning types and their schedules, the
split rule, the library's refusals that need no device, and the slicing of UNetEngine.cfm_recon on a handle-less engine.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from mi355.synth import rand_uniform, randn, synth_state_dict
from oracle import unet_ref
from tests import flow_guidance_ref as fref

NEW_SYMBOLS = ("mi355_lowres_seed", "mi355_cfm_recon_workspace_bytes", "mi355_cfm_recon_sample")
# (H, W, h, w): the shapes the gather form of D^T was derived on
ADJOINT_SHAPES = [(16, 16, 4, 4), (16, 16, 8, 8), (12, 20, 4, 10), (64, 64, 16, 16), (16, 16, 1, 1), (15, 9, 5, 3), (16, 16, 16, 16)]


def _lib():
    import __graft_entry__ as ge

    ge.build()
    from mi355 import _lib

    return _lib, _lib.lib()


def test_library_exports_the_new_symbols():
    import os
    import re

    from tests.conftest import REPO

    _l, L = _lib()
    header = open(os.path.join(REPO, "include", "mi355_sampler.h")).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in _l.SIGNATURES and hasattr(L, name) and name in declared, name
    assert L.mi355_version() == 108   # additive: new symbols only


@pytest.mark.parametrize("H,W,h,w", ADJOINT_SHAPES)
def test_gather_adjoint_is_autograd_of_interpolate(H, W, h, w):
    """<D x, r> differentiated by torch.autograd in fp64 against the gather form (source pixel (Y, X) receives from (Y // sy, X // sx) alone).
    Expected error 0; 1e-12 allowed."""
    x = randn(900 + H + w, 2, 3, H, W).double().requires_grad_()
    r = randn(901 + H + w, 2, 3, h, w).double()
    (want,) = torch.autograd.grad((F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False) * r).sum(), x)
    got = fref.lowres_DT_gather(r, H, W)
    err = float((got - want).abs().max())
    print(f"D^T gather vs autograd {H}x{W} -> {h}x{w}: max|err| {err:.3e}")
    assert err <= 1e-12


def test_seed_ref64_gradient_is_autograd():
    """lowres_seed_ref64's g_x / g_eps against autograd of the loss it states (fp64, no NaN, nothing within rounding of the clip edges)."""
    x, eps = 0.9 * randn(31, 2, 3, 12, 10).double(), 0.9 * randn(32, 2, 3, 12, 10).double()
    y = rand_uniform(33, -1, 1, 2, 3, 4, 5).double()
    for cr, cm in ((1.0, -0.6), (1.7, 1.37)):
        crf, cmf = float(torch.tensor(cr, dtype=torch.float32)), float(torch.tensor(cm, dtype=torch.float32))
        # the seed's g_eps is the cotangent of eps -> x0: d loss / d eps = -c_recipm1 g
        ref = fref.lowres_seed_ref64(x.float(), eps.float(), y.float(), cr, cm)
        x32, e32 = x.float().double(), eps.float().double()
        xr, er = x32.clone().requires_grad_(), e32.clone().requires_grad_()
        loss = fref.constraint_loss(torch.clip(crf * xr - cmf * er, -1, 1), y.float().double(), 2)
        gx, ge = torch.autograd.grad(loss.sum(), (xr, er))
        # the restatement holds k = 2 / per as the kernel does, rounded to fp32: one rounding, 2^-24 relative
        torch.testing.assert_close(ref["g_x"], gx, rtol=2.0 ** -23, atol=1e-12)
        torch.testing.assert_close(ref["g_eps"], ge, rtol=2.0 ** -23, atol=1e-12)
        torch.testing.assert_close(ref["loss"], loss.detach(), rtol=1e-9, atol=1e-12)
        frac = float(((ref["pre"] < -1) | (ref["pre"] > 1)).double().mean())
        assert 0.05 < frac < 0.8, frac


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_reference_gradient_is_a_descent_direction(mode):
    """First order: the summed constraint loss at x - e g is below the loss at x, g the reference's guidance gradient."""
    cfg = unet_ref.UNetConfig(16, 3, 32, 3, 1, (4,), channel_mult=(1, 2, 2), num_heads=2)
    from image_diffusion.unet import param_shapes

    sd = synth_state_dict(param_shapes(cfg), 2002)
    fwd = lambda x, t: unet_ref.unet_forward_diff(sd, cfg, x, t)   # noqa: E731
    x = randn(11, 2, 3, 16, 16)
    img = rand_uniform(12, -1, 1, 2, 3, 16, 16)
    y = img.clone()
    if mode == 0:
        y[:, :, 5:11, 4:10] = -2.0
    elif mode == 2:
        y = fref.lowres_D(img, (4, 4))
    t = torch.tensor(0.5)
    _, g, l0 = fref.flow_guidance_grad(fwd, x, t, y, mode)
    e = 1e-3 / float(g.abs().max())
    _, _, l1 = fref.flow_guidance_grad(fwd, x - e * g, t, y, mode)
    print(f"mode {mode}: loss {float(l0.sum()):.6f} -> {float(l1.sum()):.6f} (|g|max {float(g.abs().max()):.3e})")
    assert float(l1.sum()) < float(l0.sum())


def test_flow_recon_ref_plumbing():
    """The restatement on a toy field v = -x (no net): paste, unguided step, final paste and the trajectory."""
    fwd = lambda x, t: -x   # noqa: E731
    x0 = randn(5, 2, 1, 4, 4)
    y = rand_uniform(6, -1, 1, 2, 1, 4, 4)
    y[:, :, 1:3, 1:3] = -2.0
    ts = [0.0, 0.5, 1.0]
    out = fref.flow_recon_ref(None, None, x0, ts, y, 0, None, "coupled", True, forward=fwd)
    known = y != -2.0
    assert torch.equal(out["x"][known], y[known]) and out["traj"].shape[0] == 3 and torch.equal(out["traj"][-1], out["x"])
    plain = fref.flow_recon_ref(None, None, x0, ts, None, 0, None, None, False, forward=fwd)
    assert torch.equal(plain["x"], x0 * 0.5 * 0.5) and torch.isnan(plain["losses"]).all()
    zero = fref.flow_recon_ref(None, None, x0, ts, y, 0, [0.0, 0.0], None, False, forward=fwd)
    assert torch.equal(zero["x"], plain["x"])


def test_low_resolution_likelihood():
    from image_diffusion.likelihoods import LowResolution, get_likelihood

    lik = LowResolution(4, 8)
    x = randn(21, 3, 2, 16, 16)
    y = lik.sample(x)
    assert torch.equal(y, F.interpolate(x, size=(4, 8), mode="bilinear", align_corners=False))
    assert lik.none_like(x).shape == (3, 2, 4, 8) and not lik.none_like(x).any()
    x2 = randn(22, 3, 2, 16, 16)
    want = ((F.interpolate(x2, size=(4, 8), mode="bilinear", align_corners=False) - y) ** 2).mean(dim=(1, 2, 3))
    torch.testing.assert_close(lik.loss(x2, y), want, rtol=0, atol=0)
    assert not lik.loss(x, y).any()
    assert get_likelihood("LowResolution") is LowResolution
    assert LowResolution.from_configdict(dict(target_height=2, target_width=3)).target_width == 3


def test_conditioning_types_and_schedules():
    from image_diffusion.conditioning import (FlowReconstructionGuidance, FlowReplacement, ReconstructionGuidance, flow_split_index,
                                              get_conditioning)

    assert get_conditioning("flow_replacement") is FlowReplacement
    assert get_conditioning("flow_reconstruction_guidance") is FlowReconstructionGuidance
    r = FlowReplacement(0.5, "coupled")
    assert (r.start_fraction, r.noise) == (0.5, "coupled")
    assert FlowReplacement.from_configdict(dict(start_fraction=1.0, noise="fresh")).noise == "fresh"
    with pytest.raises(ValueError):
        FlowReplacement(1.0, "white")
    g = FlowReconstructionGuidance(0.3, 1.0, "constant", None)
    assert (g.gamma, g.start_fraction, g.schedule, g.replace) == (0.3, 1.0, "constant", None)
    with pytest.raises(ValueError):
        FlowReconstructionGuidance(0.3, 1.0, "linear", None)
    with pytest.raises(ValueError):
        FlowReconstructionGuidance(0.3, 1.0, "constant", "white")
    with pytest.raises(TypeError):
        FlowReconstructionGuidance(0.3, 1.0)
    ts = [float(v) for v in torch.linspace(0, 1, 7)][:-1]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)   # noqa: E731
    assert g.scales(ts) == [float(f32(0.3))] * 6
    om = FlowReconstructionGuidance(0.3, 1.0, "one_minus_t", None).scales(ts)
    assert om == [float(f32(0.3) * (f32(1.0) - f32(t))) for t in ts]
    fn = FlowReconstructionGuidance(0.3, 1.0, lambda t: 2.0 * t * t + 0.1, "coupled").scales(ts)
    assert fn == [float(f32(2.0 * float(f32(t)) ** 2 + 0.1)) for t in ts]
    for s in g.scales(ts) + om + fn:
        assert float(f32(s)) == s   # fp32 values
    assert [flow_split_index(6, f) for f in (0, 0.5, 1)] == [0, 3, 6]
    assert [flow_split_index(7, f) for f in (0, 0.5, 1)] == [0, 3, 7]
    assert "not built yet" not in ReconstructionGuidance.__doc__


def test_library_refusals_without_a_device():
    _l, L = _lib()
    host = (C.c_float * 4096)()                 # host memory that no launch ever sees: every call below is refused first
    p = C.cast(host, C.c_void_p)
    # lowres_seed: null pointers, then the shape rule
    assert L.mi355_lowres_seed(None, p, p, 1.0, -0.5, 1, 1, 16, 16, 4, 4, p, p, p, None, None) == -1
    assert L.mi355_lowres_seed(p, p, p, 1.0, -0.5, 1, 1, 16, 16, 4, 4, p, None, p, None, None) == -1
    for H, W, h, w in ((16, 16, 5, 4), (16, 16, 4, 3), (15, 9, 4, 3), (16, 16, 32, 32)):
        assert L.mi355_lowres_seed(p, p, p, 1.0, -0.5, 1, 1, H, W, h, w, p, p, p, None, None) == -4, (H, W, h, w)   # MI355_ERR_UNSUPPORTED
        assert b"integer factors" in L.mi355_last_error()
    assert L.mi355_lowres_seed(p, p, p, 1.0, -0.5, 1, 1, 16, 16, 0, 4, p, p, p, None, None) == -1
    # the sampler: null handle / state / span, n_t < 1, mode 3, replace with mode 2, final_paste without replace - before the handle is read
    ts = (C.c_float * 3)(0.0, 0.5, 1.0)

    def call(net=p, x=p, n_t=3, y=p, mode=0, replace=0, final_paste=0, batch=1):
        return L.mi355_cfm_recon_sample(net, x, 3, None, ts, n_t, y, mode, -2.0, 4, 4, None, replace, final_paste, None, 0, None, None, None, batch, p,
                                        4096, None)

    assert call(net=None) == -1 and call(x=None) == -1 and call(batch=0) == -1
    assert call(n_t=0) == -1 and b"n_t >= 1" in L.mi355_last_error()
    assert call(mode=3) == -1 and b"mode" in L.mi355_last_error()
    assert call(mode=-1) == -1
    assert call(mode=2, replace=1) == -1 and b"replacement" in L.mi355_last_error()
    assert call(mode=1, replace=2) == -1
    assert call(replace=3) == -1
    assert call(final_paste=1) == -1 and b"final_paste" in L.mi355_last_error()
    assert L.mi355_cfm_recon_workspace_bytes(None, 4, 4, 4) < 0


def _fake_engine(max_batch=64, differentiable=True, num_classes=0):
    from mi355.engine import UNetEngine

    class Rec(UNetEngine):
        def __init__(self):   # no device, no handle
            self.device = torch.device("cpu")
            self.num_classes, self.in_channels, self.out_channels, self.image_size = num_classes, 3, 3, 8
            self.max_batch_override = max_batch
            self.differentiable = differentiable
            self.calls = []

        def __del__(self):
            pass

        def _cfm_recon_call(self, x, ts, y, mode, scales, rep, final_paste, pad_value, noise, seed, lab, traj, u8, loss, hl, wl):
            self.calls.append(dict(B=x.shape[0], y=None if y is None else y.clone(), noise=None if noise is None else noise.clone(), seed=seed,
                                   lab=None if lab is None else lab.clone(), rep=rep, scales=scales, hl=hl, wl=wl, mode=mode, fp=final_paste))
            x += 1.0
            if traj is not None:
                traj.copy_(x.expand_as(traj))
            if loss is not None:
                loss.fill_(float(x.shape[0]))

    return Rec()


def test_cfm_recon_host_logic_and_slicing():
    from mi355._lib import MI355BackendError

    x = torch.zeros(5, 3, 8, 8)
    ts = [0.0, 0.5, 1.0]
    y = torch.arange(5.0).view(5, 1, 1, 1).expand(5, 3, 8, 8).contiguous()
    eng = _fake_engine(max_batch=2)
    noise = torch.arange(15.0).view(3, 5, 1, 1, 1).expand(3, 5, 3, 8, 8).contiguous()
    out, traj, u8, loss = eng.cfm_recon(x, ts, y, 0, scales=[0.5, 0.25], replace="fresh", final_paste=True, noise=noise, keep_traj=True)
    assert [c["B"] for c in eng.calls] == [2, 2, 1] and bool((out == 1).all()) and traj.shape == (3, 5, 3, 8, 8) and loss is None
    for i, (lo, hi) in enumerate(((0, 2), (2, 4), (4, 5))):
        c = eng.calls[i]
        assert torch.equal(c["y"], y[lo:hi]) and torch.equal(c["noise"], noise[:, lo:hi]) and c["rep"] == 2 and c["fp"] and c["scales"] == [0.5, 0.25]
    # Philox: each slice its own key; mode 2 carries the low resolution and returns the per-slice losses
    eng = _fake_engine(max_batch=2)
    ylow = torch.zeros(5, 3, 2, 4)
    _, _, _, loss = eng.cfm_recon(torch.zeros(5, 3, 8, 8), ts, ylow, 2, scales=[1.0, 0.0], return_loss=True, seed=7)
    assert [(c["hl"], c["wl"]) for c in eng.calls] == [(2, 4)] * 3 and loss.shape == (2, 5) and loss[0].tolist() == [2, 2, 2, 2, 1]
    eng = _fake_engine(max_batch=2)
    eng.cfm_recon(torch.zeros(3, 3, 8, 8), ts, torch.zeros(3, 3, 8, 8), 0, replace="fresh", seed=7)
    assert [c["seed"] for c in eng.calls] == [7, 8]
    # refusals before any call
    eng = _fake_engine(differentiable=False)
    with pytest.raises(MI355BackendError, match="differentiable"):
        eng.cfm_recon(x, ts, y, 0, scales=[0.5, 0.0])
    eng.cfm_recon(torch.zeros(5, 3, 8, 8), ts, y, 0, scales=[0.0, 0.0])   # all-zero scales need no backward
    eng.cfm_recon(torch.zeros(5, 3, 8, 8), ts, y, 0, replace="coupled")   # pure replacement: any engine
    assert len(eng.calls) == 2
    eng = _fake_engine()
    for kw, exc in ((dict(mode=3), ValueError), (dict(replace="white"), ValueError), (dict(scales=[1.0]), ValueError),
                    (dict(return_loss=True), ValueError), (dict(noise=noise), ValueError), (dict(y=torch.zeros(5, 3, 4, 4)), ValueError),
                    (dict(y_labels=torch.zeros(5, dtype=torch.long)), ValueError)):
        args = dict(y=y, mode=0)
        args.update(kw)
        with pytest.raises(exc):
            eng.cfm_recon(x, ts, args.pop("y"), args.pop("mode"), **args)
    assert not eng.calls


def test_flow_sample_fn_refusals():
    from flow_sampling import get_flow_conditional_sample_fn
    from image_diffusion.conditioning import FlowReconstructionGuidance, FlowReplacement, Replacement
    from image_diffusion.likelihoods import HyperResolution, InPainting
    from image_diffusion.unet import UNetModel
    from mi355._lib import MI355BackendError

    net = UNetModel(image_size=16, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=(4,),
                    channel_mult=(1, 2, 2), num_heads=2, precision="fp32")
    ts = torch.linspace(0, 1, 5).tolist()
    lik = InPainting(6, -2.0)
    sample = get_flow_conditional_sample_fn(net, FlowReconstructionGuidance(0.5, 1.0, "constant", None), lik, ts)
    with pytest.raises(MI355BackendError):
        sample(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16))          # CPU tensors: no fallback
    with pytest.raises(MI355BackendError):
        get_flow_conditional_sample_fn(net, FlowReplacement(1.0, "coupled"), lik, ts)(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16))
    with pytest.raises(NotImplementedError):
        get_flow_conditional_sample_fn(lambda t, x: x, FlowReplacement(1.0, "coupled"), lik, ts)   # an arbitrary callable has no engine
    with pytest.raises(NotImplementedError):
        get_flow_conditional_sample_fn(net, Replacement(0.1, 1.0, True, 0), lik, ts)               # a diffusion conditioning type
    with pytest.raises(ValueError):
        get_flow_conditional_sample_fn(net, FlowReplacement(1.0, "coupled"), HyperResolution(4, 4), ts)   # nothing to paste
    with pytest.raises(ValueError):
        get_flow_conditional_sample_fn(net, FlowReplacement(1.0, "coupled"), lik, [0.0])
