"""CPU: the host side of classifier-free guidance - the new symbols, the Python surface's refusals (before any device work), the
conditioning type, the generic sampler's host logic on a recording op table, and the slicing rule (guided calls run at twice the batch:
slices of max_batch() // 2 that carry their labels, conditions and scales; max_batch() = 1 cannot hold a guided evaluation and is refused).

The library's own host-only refusals and its workspace rule need a handle, and a handle needs a device (mi355_unet_create uploads the
weights): they are in tests/test_gpu_cfg.py::test_workspace_rule_and_refusals.
"""
import inspect

import pytest
import torch

NEW_SYMBOLS = ("mi355_cfg_workspace_bytes", "mi355_cfm_cfg_sample", "mi355_ddpm_cfg_workspace_bytes", "mi355_ddpm_cfg_sample", "mi355_cfg_stage",
               "mi355_ddpm_cfg_step", "mi355_ddim_cfg_step")


def test_library_exports_the_new_symbols():
    import __graft_entry__ as ge

    ge.build()
    from mi355 import _lib

    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.mi355_version() == 108   # additive: new symbols only
    # the size functions refuse a null handle and a bad stage count on the host
    assert L.mi355_cfg_workspace_bytes(None, 4, 1) < 0 and L.mi355_ddpm_cfg_workspace_bytes(None, 4) < 0
    assert b"stages" in L.mi355_last_error() or b"bad argument" in L.mi355_last_error()
    # and the samplers a null handle, before anything else
    assert L.mi355_cfm_cfg_sample(None, None, 1, None, 0, -2.0, None, 0, 1.0, None, None, 0, 1, None, None, None, None, None, 1, None, 0, None) < 0
    assert L.mi355_ddpm_cfg_sample(None, None, 1, None, None, 0, 1.0, None, None, None, None, 0, 1, None, 0, None) < 0


def _fake_engine(num_classes=10, in_channels=1, out_channels=1, size=8, max_batch=None):
    """A UNetEngine without a handle: the guided methods' host logic up to the library call, which is recorded instead."""
    from mi355.engine import UNetEngine

    class Rec(UNetEngine):
        def __init__(self):   # no device, no handle
            self.device = torch.device("cpu")
            self.num_classes, self.in_channels, self.out_channels, self.image_size = num_classes, in_channels, out_channels, size
            self.max_batch_override = max_batch
            self.calls = []

        def __del__(self):
            pass

        def _cfm_cfg_call(self, x, ts, tableau, cond, lab, null_label, w, wt, none_value, traj, u8):
            self.calls.append(dict(B=x.shape[0], x=x.clone(), cond=None if cond is None else cond.clone(), lab=None if lab is None else lab.clone(),
                                   null=null_label, w=w, wt=None if wt is None else wt.clone(), stages=len(tableau[1]), none=none_value))
            x += 1.0
            if traj is not None:
                traj.copy_(x.expand_as(traj))
            if u8 is not None:
                u8.fill_(7)

        def _ddpm_cfg_call(self, x, tables, mode, cond, lab, null_label, w, wt, noise, o):
            self.calls.append(dict(B=x.shape[0], lab=None if lab is None else lab.clone(), wt=None if wt is None else wt.clone(), w=w,
                                   noise=None if noise is None else noise.clone(), cond=cond.clone(), seed=o["seed"], null=null_label))
            x += 1.0

    return Rec()


def test_python_refusals_before_device_work():
    from mi355 import _lib

    eng = _fake_engine()
    x = torch.zeros(2, 1, 8, 8)
    y = torch.tensor([1, 2])
    ts = [0.0, 0.5, 1.0]
    for bad in (10, -1):
        with pytest.raises(ValueError, match="null_label"):
            eng.cfm_euler(x, ts, y=y, guidance_scale=2.0, null_label=bad)
    with pytest.raises(ValueError, match="something to guide"):
        eng.cfm_euler(x, ts, guidance_scale=2.0)
    with pytest.raises(ValueError, match="something to guide"):
        eng.cfm_rk(x, ts, "rk4", guidance_scale=0.0)   # any float takes the guided path, 0 included
    with pytest.raises(ValueError, match="without num_classes"):
        _fake_engine(num_classes=0).cfm_euler(x, ts, y=y, guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="cond_drift"):
        _fake_engine(in_channels=2).cfm_euler(x, ts, cond=x, cond_drift=True, guidance_scale=2.0)
    with pytest.raises(ValueError, match="shape"):
        eng.cfm_euler(x, ts, y=y, guidance_scale=torch.ones(3))
    with pytest.raises(ValueError):
        eng.cfm_rk(x, ts, ([[]] * 5, [0.2] * 5, [0] * 5), y=y, guidance_scale=2.0)   # five stages
    e2 = _fake_engine(num_classes=0, in_channels=2)
    for mode in (_lib.DDPM_PRIOR, _lib.DDPM_REPLACEMENT):
        with pytest.raises(NotImplementedError, match="prior and replacement"):
            e2.ddpm_sample(x, {}, mode=mode, cond=x, guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="guided path"):
        e2.ddpm_sample(x, {}, mode=_lib.DDPM_AMORTIZED, cond=x, y=y)
    assert not eng.calls and not e2.calls
    # every addition is a trailing keyword that defaults to today's behaviour
    from mi355.engine import UNetEngine

    for fn in (UNetEngine.forward, UNetEngine.cfm_euler, UNetEngine.cfm_rk, UNetEngine.ddpm_sample):
        p = inspect.signature(fn).parameters
        assert p["guidance_scale"].default is None and p["null_label"].default is None
    assert list(inspect.signature(UNetEngine.cfm_rk).parameters)[:8] == ["self", "x", "t_span", "method", "cond", "keep_traj", "want_u8", "y"]


@pytest.mark.parametrize("override,sizes", [(None, [7]), (3, [1] * 7), (2, [1] * 7), (4, [2, 2, 2, 1]), (13, [6, 1]), (14, [7])])
def test_slicing_rule(override, sizes):
    """Guided batches are cut at max_batch() // 2; every slice gets its own labels, condition rows and scales."""
    eng = _fake_engine(num_classes=10, in_channels=2, max_batch=override or 1000)
    B = 7
    x = torch.arange(B, dtype=torch.float32).reshape(B, 1, 1, 1).expand(B, 1, 8, 8).contiguous()
    cond = -x.clone()
    y = torch.arange(B) % 9
    wt = torch.arange(B, dtype=torch.float32) / 2
    assert eng.cfg_batch() == (override or 1000) // 2
    x_in = x.clone()
    _, traj, u8 = eng.cfm_rk(x, [0.0, 0.5, 1.0], "rk4", cond=cond, y=y, guidance_scale=wt, keep_traj=True, want_u8=True, none_value=0.0)
    assert [c["B"] for c in eng.calls] == sizes
    lo = 0
    for c in eng.calls:
        hi = lo + c["B"]
        assert torch.equal(c["x"], x_in[lo:hi]) and torch.equal(c["cond"], cond[lo:hi])
        assert torch.equal(c["lab"], y[lo:hi].to(torch.int32)) and torch.equal(c["wt"], wt[lo:hi])
        assert c["null"] == 9 and c["stages"] == 4 and c["none"] == 0.0   # null_label defaults to the last class
        lo = hi
    assert torch.equal(x, x_in + 1) and traj.shape == (3, B, 1, 8, 8) and torch.equal(traj[1], x) and (u8 == 7).all()
    # a float scale; Euler is the one-stage tableau
    eng.calls.clear()
    eng.cfm_euler(x, [0.0, 1.0], cond=cond, guidance_scale=0)
    assert [c["B"] for c in eng.calls] == sizes and all(c["w"] == 0.0 and c["wt"] is None and c["lab"] is None and c["stages"] == 1 for c in eng.calls)
    # the DDPM path: injected draws are cut along the batch axis, Philox seeds differ per slice
    from mi355 import _lib

    eng.calls.clear()
    noise = torch.arange(3 * B, dtype=torch.float32).reshape(3, B, 1, 1, 1).expand(3, B, 1, 8, 8).contiguous()
    xd = x.clone()
    eng.ddpm_sample(xd, {}, mode=_lib.DDPM_AMORTIZED, cond=cond, noise=noise, guidance_scale=wt, y=y, null_label=0, seed=5)
    assert [c["B"] for c in eng.calls] == sizes and torch.equal(xd, x + 1)
    lo = 0
    for i, c in enumerate(eng.calls):
        hi = lo + c["B"]
        assert torch.equal(c["noise"], noise[:, lo:hi]) and torch.equal(c["cond"], cond[lo:hi]) and torch.equal(c["wt"], wt[lo:hi])
        assert c["seed"] == 5 + i and c["null"] == 0
        lo = hi


def test_max_batch_of_one_is_refused():
    """A guided evaluation is two images: an engine limited to one refuses every guided entry point in Python, before any library call, and
    its unguided limit is untouched."""
    from mi355 import _lib
    from mi355._lib import MI355BackendError

    eng = _fake_engine(num_classes=10, in_channels=2, max_batch=1)
    x = torch.zeros(1, 1, 8, 8)
    y = torch.tensor([3])
    with pytest.raises(MI355BackendError, match="max_batch"):
        eng.cfg_batch()
    with pytest.raises(MI355BackendError, match="max_batch"):
        eng.cfm_euler(x, [0.0, 1.0], cond=x, y=y, guidance_scale=2.0)
    with pytest.raises(MI355BackendError, match="max_batch"):
        eng.cfm_rk(x, [0.0, 1.0], "rk4", cond=x, guidance_scale=2.0)
    with pytest.raises(MI355BackendError, match="max_batch"):
        eng.ddpm_sample(x, {}, mode=_lib.DDPM_AMORTIZED, cond=x, guidance_scale=2.0)
    with pytest.raises(MI355BackendError, match="max_batch"):
        eng.forward(x, 0.5, cond=x, guidance_scale=2.0)
    assert not eng.calls and torch.equal(x, torch.zeros_like(x)) and eng.max_batch() == 1


def test_conditioning_type():
    from image_diffusion.conditioning import Amortized, ClassifierFreeGuidance, get_conditioning

    assert get_conditioning("classifier_free_guidance") is ClassifierFreeGuidance
    assert ClassifierFreeGuidance.KEY == "classifier_free_guidance"
    assert ClassifierFreeGuidance.PARAMS == Amortized.PARAMS + ("guidance_scale",)
    c = ClassifierFreeGuidance(0.8, 2, 0.05, 3.0)   # positionally, in PARAMS order
    assert (c.p_cond, c.n_corrector, c.delta, c.guidance_scale) == (0.8, 2, 0.05, 3.0) and isinstance(c, Amortized)
    assert ClassifierFreeGuidance.from_configdict(dict(p_cond=0.8, n_corrector=0, delta=0.1, guidance_scale=1.5, extra=1)).guidance_scale == 1.5
    with pytest.raises(TypeError):
        ClassifierFreeGuidance(0.8, 2, 0.05)
    with pytest.raises(TypeError):
        ClassifierFreeGuidance(0.8, 2, 0.05, 3.0, 1)
    assert get_conditioning("amortized") is Amortized


class _RecOps:
    """The step ops in eager torch (CPU), recording what the generic guided sampler asks for."""

    def __init__(self):
        self.log = []

    def cfg_combine(self, v2, w, out=None):
        B = v2.shape[0] // 2
        self.log.append(("cfg_combine", float(w)))
        d = v2[:B] - v2[B:]
        return v2[B:] + d * w

    def ddpm_step_(self, x, eps, z, c_recip, c_recipm1, coef1, coef2, sigma, philox=None):
        self.log.append(("ddpm_step", z is not None))
        x0 = (c_recip * x - c_recipm1 * eps).clip(-1, 1)
        x.copy_(coef1 * x0 + coef2 * x + (sigma * z if z is not None else 0))
        return x

    def corrector_step_(self, x, eps, z, *a, **k):
        self.log.append(("corrector", True))
        return x

    def ddim_step_(self, x, eps, *a):
        self.log.append(("ddim_step", False))
        return x

    def clip_(self, x, lo=-1.0, hi=1.0):
        return x.clip_(lo, hi)


def test_generic_guided_sampler_host_logic():
    """Two eps_model calls per predictor step (the condition, then none_like), one cfg_combine, the predictor; the corrector sees none_like;
    dispatched before Amortized."""
    from image_diffusion import sampling
    from image_diffusion.conditioning import ClassifierFreeGuidance
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM

    ddpm = DDPM(25)
    lik = InPainting(patch_size=3, pad_value=-2)
    seen = []

    def eps_model(xi, i):
        seen.append(float(xi[:, 1:].mean()))   # the condition channel
        return xi[:, :1] * 0.1 + xi[:, 1:] * 0.01

    xT = torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(1))
    cond = torch.full_like(xT, 0.5)
    rec = _RecOps()
    draws = [torch.zeros_like(xT)] * (2 * 25)
    with sampling.use_ops(rec), sampling.injected_noise(draws):
        out = sampling.get_conditional_sample_fn(eps_model, ddpm, ClassifierFreeGuidance(0.9, 1, 0.1, 2.5), lik)(xT, cond)
    assert out.shape == xT.shape and torch.isfinite(out).all()
    assert seen == [0.5, -2.0, -2.0] * 25
    assert rec.log[:3] == [("cfg_combine", 2.5), ("ddpm_step", True), ("corrector", True)] and len(rec.log) == 3 * 25
    assert rec.log[-2] == ("ddpm_step", False)   # i == 0: no noise
    rec.log.clear()
    seen.clear()
    with sampling.use_ops(rec):
        sampling.get_ddim_sample_fn(eps_model, ddpm, lik, guidance_scale=2.5)(xT, cond)
        with pytest.raises(ValueError, match="condition"):
            sampling.get_ddim_sample_fn(eps_model, ddpm, lik, guidance_scale=2.5)(xT)
    assert rec.log == [("cfg_combine", 2.5), ("ddim_step", False)] * 25 and seen == [0.5, -2.0] * 25
    assert inspect.signature(sampling.get_ddim_sample_fn).parameters["guidance_scale"].default is None


def test_compat_surface():
    import compute_fid
    from torchcfm_compat import GuidedVectorField, UNetModelWrapper

    p = inspect.signature(UNetModelWrapper.forward).parameters
    assert list(p)[:4] == ["self", "t", "x", "y"] and p["guidance_scale"].default is None and p["null_label"].default is None
    with pytest.raises(ValueError):
        GuidedVectorField(object())
    f = GuidedVectorField(object(), y=torch.tensor([1]), guidance_scale=2.0)
    assert f.none_value == -2.0 and f.null_label is None
    with pytest.raises(ValueError, match="class-conditional"):
        compute_fid.make_gen_1_img(type("N", (), {"num_classes": None})(), guidance_scale=2.0, device="cpu")
    with pytest.raises(ValueError, match="null_label"):
        compute_fid.make_gen_1_img(type("N", (), {"num_classes": 11})(), guidance_scale=2.0, null_label=11, device="cpu")
    assert callable(compute_fid.make_gen_1_img(type("N", (), {"num_classes": 11})(), guidance_scale=2.0, device="cpu"))
