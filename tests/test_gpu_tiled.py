"""GPU: tiled sampling (MultiDiffusion) on the HIP path - the two kernels bit for bit against slicing and against the eager fp32 blend, one tiled
evaluation against the fp64 restatement (tests/tiled_ref.py) in all four precisions, chunked evaluation, the tiled Euler and DDPM samplers against
the restated loops, the Python surface and every refusal.

Tolerances are the project's own for the same arithmetic, unchanged, because the blend is a convex combination of window outputs: the forward's
fp32 bound rtol 2e-4 / atol 5e-5 and bf16 bound err < 0.04 * scale, rms < 0.02 (tests/test_gpu_unet.py::test_unet_forward_fp32 / _bf16, as
tests/test_gpu_feature_cache.py uses them); the Euler-trajectory bound 5e-4 / 5e-5 (tests/test_gpu_feature_cache.py::test_cached_euler); the bf16
Euler bound err < 0.08, rms < 0.015 (tests/test_gpu_unet.py::test_cifar_cfm_euler_bf16_vs_fp32_oracle); SAMPLER_TOL for the DDPM loops
(tests/test_gpu_unet.py).  A wrong tiling (last window wins, the other weight, another stride) is off by 0.55 to 0.75 at an output scale of 3.7
(tests/test_tiled_cpu.py::test_discrimination).
"""
import ctypes as C
import functools

import pytest
import torch

from mi355.synth import randn
from oracle import cfm_ref
from tests import tiled_ref as R
from tests.test_feature_cache_cpu import TINY, tiny_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAMPLER_TOL = dict(rtol=2e-3, atol=1e-3)   # tests/test_gpu_unet.py
B2, S = 2, 16
HW, STRIDE = (24, 40), (5, 7)   # 3 x 5 = 15 windows per canvas, the last row and column clamped, rows starting at unaligned canvas columns
T_EVAL = 0.3


@functools.lru_cache(maxsize=None)
def _net(idx, precision):
    from tests.test_gpu_unet import build

    return build(TINY[idx], 1003, precision)[0]


@functools.lru_cache(maxsize=None)
def _cond_net(precision="fp32"):
    from tests.test_gpu_unet import _tiny

    return _tiny(6, 3, 1006, precision)   # (cfg, net, sd): a 2C-input net


def _canvas(seed, c=3, hw=HW, b=B2):
    return randn(seed, b, c, *hw)


def _report(tag, got, ref):
    err = (got.double() - ref.double()).abs()
    scale = float(ref.abs().max())
    rms = float(err.pow(2).mean().sqrt()) / max(float(ref.double().pow(2).mean().sqrt()), 1e-12)
    print(f"{tag}: max|err| {float(err.max()):.3e} (scale {scale:.3f}), rel rms {rms:.3e}")
    return float(err.max()), scale, rms


def _forward_bound(precision, got, ref, tag):
    err, scale, rms = _report(tag, got, ref)
    if precision == "fp32":
        torch.testing.assert_close(got.double(), ref.double(), rtol=2e-4, atol=5e-5)
    else:
        assert err < 0.04 * scale and rms < 0.02


# ---- 1. op level, no U-Net -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw,stride,n_windows", [((17, 18), (1, 1), 6), ((24, 40), (5, 7), 15)])
def test_tile_gather_is_slicing(hw, stride, n_windows):
    from mi355.engine import tile_plan
    from mi355.ops import default_ops

    tp = tile_plan(S, hw, stride)
    assert tp["n_windows"] == n_windows
    x = _canvas(21, 3, hw)
    got = default_ops.tile_gather(x.to(DEV), S, tp)
    assert torch.equal(got.cpu(), R.cut(x, S, stride))


@pytest.mark.parametrize("euler", [False, True])
@pytest.mark.parametrize("weight", ["uniform", "tent"])
@pytest.mark.parametrize("hw,stride", [((17, 18), (1, 1)), ((24, 40), (5, 7))])
def test_tile_blend_is_the_eager_fp32_expression(hw, stride, weight, euler):
    """Bit for bit: ascending windows, num += w * v, den += w, num / den, x + dt * vbar (the eager expression evaluated on the CPU)."""
    from mi355.engine import tile_plan
    from mi355.ops import default_ops

    tp = tile_plan(S, hw, stride, weight)
    v = randn(22, B2 * tp["n_windows"], 3, S, S)
    x, dt = _canvas(23, 3, hw), 0.37
    plan = dict(canvas_hw=hw, stride=stride, weight=weight)
    if euler:
        want_v, want_x = R.blend_fp32(v, plan, x, dt)
        xd = x.to(DEV).clone()
        got = default_ops.tile_blend_(v.to(DEV), tp, x=xd, dt=dt)
        assert torch.equal(xd.cpu(), want_x)
    else:
        want_v = R.blend_fp32(v, plan)
        got = default_ops.tile_blend_(v.to(DEV), tp)
    assert torch.equal(got.cpu(), want_v)


def test_tile_labels_repeat():
    from mi355.ops import default_ops

    y = torch.tensor([3, 0, 4], dtype=torch.int32)
    assert torch.equal(default_ops.tile_labels(y.to(DEV), 15).cpu(), y.repeat_interleave(15))


# ---- 2. one tiled evaluation against the fp64 restatement ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ref_eval(idx, weight):
    return R.tiled_eval(tiny_sd(idx), TINY[idx], _canvas(31), T_EVAL, STRIDE, weight)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("idx,weight", [(0, "uniform"), (1, "tent")])
def test_forward_tiled_vs_restatement(idx, weight, precision):
    eng = _net(idx, precision).engine(DEV)
    got = eng.forward_tiled(_canvas(31).to(DEV), T_EVAL, tiling=dict(stride=STRIDE, weight=weight))
    eng.check()
    assert got.shape == (B2, 3, *HW)
    _forward_bound(precision, got.cpu(), _ref_eval(idx, weight), f"net {idx} {precision} {weight}: tiled forward vs restatement")


@pytest.mark.parametrize("precision", ["bf16x2", "fp16"])
def test_forward_tiled_other_precisions(precision):
    eng = _net(0, precision).engine(DEV)
    got = eng.forward_tiled(_canvas(31).to(DEV), T_EVAL, tiling=dict(stride=STRIDE, weight="uniform"))
    eng.check()
    _forward_bound(precision, got.cpu(), _ref_eval(0, "uniform"), f"{precision}: tiled forward vs restatement")


def test_forward_tiled_in_chunks():
    """chunk=4: 30 windows in 8 forwards, the last of 2, held to the same bound; the unchunked call is one forward of 30."""
    eng = _net(0, "fp32").engine(DEV)
    x = _canvas(31).to(DEV)
    whole = eng.forward_tiled(x, T_EVAL, tiling=dict(stride=STRIDE, weight="uniform"))
    n_whole = eng.stats(B2)["launches"]
    got = eng.forward_tiled(x, T_EVAL, tiling=dict(stride=STRIDE, weight="uniform", chunk=4))
    n_chunked = eng.stats(B2)["launches"]
    eng.check()
    print(f"max |chunked - unchunked| {float((got - whole).abs().max()):.3e}; launches {n_whole} whole, {n_chunked} in 8 chunks")
    _forward_bound("fp32", got.cpu(), _ref_eval(0, "uniform"), "chunk=4: tiled forward vs restatement")
    assert n_chunked > n_whole   # 8 forwards + 2 against 1 forward + 2


def test_forward_tiled_with_labels(golden):
    from tests.test_classcond_cpu import load_case
    from tests.test_gpu_classcond import _model

    g, cfg = load_case(golden, "tiny")
    net, sd = _model(cfg, int(g["seed"]), "fp32")
    eng = net.engine(DEV)
    x, y = _canvas(32), torch.tensor([1, cfg.num_classes - 1])
    ref = R.tiled_eval(sd, cfg, x, T_EVAL, STRIDE, "tent", y=y)
    other = R.tiled_eval(sd, cfg, x, T_EVAL, STRIDE, "tent", y=y.flip(0))
    got = eng.forward_tiled(x.to(DEV), T_EVAL, y=y.to(DEV), tiling=dict(stride=STRIDE, weight="tent", chunk=7))
    eng.check()
    print(f"   (the other canvas's labels would be off by {float((other - ref).abs().max()):.2f})")
    _forward_bound("fp32", got.cpu(), ref, "labels: tiled forward vs restatement")


def test_forward_tiled_with_condition_canvas():
    cfg, net, sd = _cond_net()
    eng = net.engine(DEV)
    x, cond = _canvas(33), _canvas(34)
    ref = R.tiled_eval(sd, cfg, x, T_EVAL, STRIDE, "uniform", cond=cond)
    got = eng.forward_tiled(x.to(DEV), T_EVAL, cond=cond.to(DEV), tiling=dict(stride=STRIDE, chunk=11))
    eng.check()
    _forward_bound("fp32", got.cpu(), ref, "condition canvas: tiled forward vs restatement")


# ---- 3. the tiled Euler sampler ------------------------------------------------------------------------------------------------------------------

TS = [0.0, 0.25, 0.5, 0.75, 1.0]


@functools.lru_cache(maxsize=None)
def _ref_euler(idx, weight):
    return R.tiled_euler(tiny_sd(idx), TINY[idx], _canvas(41), torch.tensor(TS), STRIDE, weight)


@pytest.mark.parametrize("idx,weight,chunk", [(0, "uniform", None), (1, "tent", 8)])
def test_tiled_euler_fp32(idx, weight, chunk):
    eng = _net(idx, "fp32").engine(DEV)
    ref = _ref_euler(idx, weight)
    x, traj, u8 = eng.cfm_euler(_canvas(41).to(DEV), TS, keep_traj=True, want_u8=True, tiling=dict(stride=STRIDE, weight=weight, chunk=chunk))
    eng.check()
    _report(f"net {idx} {weight} chunk {chunk}: tiled Euler vs fp64 restatement", traj.cpu(), ref)
    torch.testing.assert_close(traj.cpu().double(), ref, rtol=5e-4, atol=5e-5)
    assert torch.equal(x, traj[-1])
    assert torch.equal(u8.cpu(), cfm_ref.to_uint8(x.cpu()))


def test_tiled_euler_bf16():
    eng = _net(0, "bf16").engine(DEV)
    ref = _ref_euler(0, "uniform")[-1]
    x, _, _ = eng.cfm_euler(_canvas(41).to(DEV), TS, tiling=dict(stride=STRIDE))
    eng.check()
    err = (x.cpu().double() - ref).abs()
    print(f"bf16 tiled Euler: max|err| {float(err.max()):.3e} rms {float(err.pow(2).mean().sqrt()):.3e}; |x| max {float(ref.abs().max()):.2f}")
    assert err.max() < 0.08 and err.pow(2).mean().sqrt() < 0.015


def test_canvas_of_the_nets_size_is_the_untiled_sampler():
    eng = _net(0, "fp32").engine(DEV)
    x0 = randn(42, B2, 3, S, S)
    _, plain, _ = eng.cfm_euler(x0.to(DEV), TS, keep_traj=True)
    _, tiled, _ = eng.cfm_euler(x0.to(DEV), TS, keep_traj=True, tiling=dict(stride=8, weight="tent"))
    eng.check()
    _report("one window: tiled Euler vs untiled Euler", tiled, plain)
    torch.testing.assert_close(tiled, plain, rtol=5e-4, atol=5e-5)


def test_tiled_euler_with_labels_and_condition(golden):
    from tests.test_classcond_cpu import load_case
    from tests.test_gpu_classcond import _model

    g, ccfg = load_case(golden, "tiny")
    net, sd = _model(ccfg, int(g["seed"]), "fp32")
    x0, y = _canvas(43), torch.tensor([2, 0])
    ref = R.tiled_euler(sd, ccfg, x0, torch.tensor(TS), STRIDE, "uniform", y=y)
    _, traj, _ = net.engine(DEV).cfm_euler(x0.to(DEV), TS, keep_traj=True, y=y.to(DEV), tiling=dict(stride=STRIDE, chunk=13))
    net.engine(DEV).check()
    _report("labels: tiled Euler vs fp64 restatement", traj.cpu(), ref)
    torch.testing.assert_close(traj.cpu().double(), ref, rtol=5e-4, atol=5e-5)
    cfg, cnet, csd = _cond_net()
    cond = _canvas(44)
    ref = R.tiled_euler(csd, cfg, x0, torch.tensor(TS), STRIDE, "tent", cond=cond)
    _, traj, _ = cnet.engine(DEV).cfm_euler(x0.to(DEV), TS, cond=cond.to(DEV), keep_traj=True, tiling=dict(stride=STRIDE, weight="tent"))
    cnet.engine(DEV).check()
    _report("condition: tiled Euler vs fp64 restatement", traj.cpu(), ref)
    torch.testing.assert_close(traj.cpu().double(), ref, rtol=5e-4, atol=5e-5)


# ---- 4. the tiled DDPM samplers --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ddpm_net(cin):
    from tests.test_gpu_unet import _tiny

    return _tiny(cin, 3, 1010 + cin, "fp32")   # (cfg, net, sd)


def _ddpm_inputs():
    xT = randn(7601, B2, 3, *HW)
    cond = (randn(7602, B2, 3, *HW) * 0.5).clamp(-1, 1)
    cond[:, :, 6:17, 9:30] = -2.0
    return xT, cond


@pytest.mark.parametrize("mode", ["prior", "amortized_corr1", "replacement", "ddim", "ddim_respaced"])
def test_tiled_ddpm_vs_restatement(mode):
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, Replacement
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM

    ddpm = DDPM(100).respace(8) if mode == "ddim_respaced" else DDPM(25)
    K = ddpm.Ns
    T = {n: v.numpy() for n, v in ddpm.host_tables().items()}
    xT, cond = _ddpm_inputs()
    weight = "tent" if mode in ("replacement", "ddim") else "uniform"
    tiling = sampling.Tiling(stride=STRIDE, weight=weight, chunk=16 if mode == "prior" else None)
    cfg, net, sd = _ddpm_net(3 if mode in ("prior", "replacement") else 6)
    draws = [randn(7700 + j, B2, 3, *HW) for j in range(3 * K)]
    lik = InPainting(patch_size=6, pad_value=-2)
    fast = sampling.make_eps_model(net, ddpm)
    args = (sd, cfg, ddpm.time, T, xT, draws, STRIDE, weight)
    if mode == "prior":
        ref, used, n_eval = R.tiled_ddpm(*args, mode="prior")
        run = lambda t: sampling.get_prior_sample_fn(fast, ddpm, Replacement(0.1, 1.0, True, 0), lik, tiling=t)(xT.to(DEV))   # noqa: E731
    elif mode == "amortized_corr1":
        ref, used, n_eval = R.tiled_ddpm(*args, mode="amortized", cond=cond, amortized=True, n_corrector=1, delta=0.1, tmin=ddpm.tmin, tmax=ddpm.tmax)
        run = lambda t: sampling.get_conditional_sample_fn(fast, ddpm, Amortized(0.9, 1, 0.1), lik, tiling=t)(xT.to(DEV), cond.to(DEV))   # noqa: E731
    elif mode == "replacement":
        ref, used, n_eval = R.tiled_ddpm(*args, mode="replacement", cond=cond, start_fraction=0.75, noise_condition=True)
        run = lambda t: sampling.get_conditional_sample_fn(fast, ddpm, Replacement(0.1, 0.75, True, 0), lik, tiling=t)(xT.to(DEV), cond.to(DEV))   # noqa: E731
    else:
        ref, used, n_eval = R.tiled_ddpm(*args, mode="ddim", cond=cond, amortized=True)
        run = lambda t: sampling.get_ddim_sample_fn(fast, ddpm.with_tiling(t), lik)(xT.to(DEV), cond.to(DEV))   # noqa: E731
    assert n_eval == K * (2 if mode == "amortized_corr1" else 1)
    with sampling.injected_noise(draws[:max(used, 1)]):
        got = run(tiling).cpu()
    net.engine(DEV).check()
    assert got.shape == xT.shape
    _report(f"{mode}: tiled DDPM vs fp64 restatement", got, ref)
    torch.testing.assert_close(got.double(), ref, **SAMPLER_TOL)


def test_tiled_ddpm_philox_reproduces():
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib

    ddpm = DDPM(25)
    cfg, net, sd = _ddpm_net(3)
    eng = net.engine(DEV)
    xT, _ = _ddpm_inputs()
    kw = dict(mode=_lib.DDPM_PRIOR, tmin=ddpm.tmin, tmax=ddpm.tmax, tiling=dict(stride=STRIDE))
    a = eng.ddpm_sample(xT.to(DEV).clone(), ddpm.host_tables(), seed=4242, **kw)
    b = eng.ddpm_sample(xT.to(DEV).clone(), ddpm.host_tables(), seed=4242, **kw)
    c = eng.ddpm_sample(xT.to(DEV).clone(), ddpm.host_tables(), seed=4243, **kw)
    eng.check()
    assert torch.equal(a, b) and float((a - c).abs().max()) > 1e-2 and bool(torch.isfinite(a).all())
    assert float(a.abs().max()) <= 1.0


# ---- 5. the Python surface and the refusals --------------------------------------------------------------------------------------------------------

def test_neural_ode_with_tiling():
    from image_diffusion.sampling import Tiling
    from torchcfm_compat import NeuralODE, UNetModelWrapper

    net = UNetModelWrapper(dim=(3, S, S), num_channels=32, num_res_blocks=1, channel_mult=(1, 2), attention_resolutions="8", num_heads=2, precision="fp32")
    net.load_state_dict(tiny_sd(0))
    net.to(DEV)
    x0 = _canvas(41)
    traj = NeuralODE(net, solver="euler", tiling=Tiling(stride=STRIDE)).trajectory(x0.to(DEV), torch.tensor(TS))
    _report("NeuralODE(tiling=): trajectory vs fp64 restatement", traj.cpu(), _ref_euler(0, "uniform"))
    torch.testing.assert_close(traj.cpu().double(), _ref_euler(0, "uniform"), rtol=5e-4, atol=5e-5)


def test_workspace_rule_and_handle_refusals():
    from mi355 import _lib
    from mi355._lib import MI355BackendError

    eng = _net(0, "fp32").engine(DEV)
    L, h = eng.L, eng.handle
    x = _canvas(51).to(DEV)
    plan = _lib.TilePlanC(HW[0], HW[1], STRIDE[0], STRIDE[1], 0, 4)
    need = L.mi355_tiled_workspace_bytes(h, B2, C.byref(plan))
    rows = B2 * 15
    windows = 2 * rows * 3 * S * S * 4            # the net's input windows (x: in_channels = 3) and its output windows
    canvas = B2 * 3 * HW[0] * HW[1] * 4
    plain = L.mi355_unet_workspace_bytes(h, 4)
    print(f"tiled workspace {need} B = plain at chunk 4 ({plain}) + windows ({windows}) + canvas ({canvas}) + alignment")
    assert need >= plain + windows + canvas
    # chunk above the handle's largest batch
    big = _lib.TilePlanC(HW[0], HW[1], STRIDE[0], STRIDE[1], 0, 1 << 30)
    assert L.mi355_tiled_workspace_bytes(h, B2, C.byref(big)) == -1 and "chunk" in L.mi355_last_error().decode()
    with pytest.raises(ValueError, match="chunk.*max_batch"):
        eng.forward_tiled(x, 0.1, tiling=dict(stride=STRIDE, chunk=1 << 30))
    # a short workspace, cond_drift: refused before any launch (x is untouched)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(x)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.mi355_unet_forward_tiled(h, C.c_void_p(x.data_ptr()), 3, None, 0, 0.1, None, C.c_void_p(out.data_ptr()), B2, C.byref(plan),
                                    C.c_void_p(ws.data_ptr()), need - 256, stream)
    assert rc == -2 and "workspace too small" in L.mi355_last_error().decode() and "unet_forward_tiled" in L.mi355_last_error().decode()
    ts = (C.c_float * 3)(0.0, 0.5, 1.0)
    before = x.clone()
    rc = L.mi355_cfm_euler_sample_tiled(h, C.c_void_p(x.data_ptr()), 3, None, 0, 1, None, ts, 3, None, None, B2, C.c_void_p(ws.data_ptr()), need, stream,
                                        C.byref(plan))
    assert rc == -4 and "cond_drift" in L.mi355_last_error().decode()
    for bad, word in (((15, 40, 8, 8, 0, 4), "canvas_h"), ((24, 40, 8, 17, 0, 4), "stride_x"), ((24, 40, 8, 8, 5, 4), "weight"),
                      ((24, 40, 8, 8, 0, 0), "chunk")):
        p = _lib.TilePlanC(*bad)
        rc = L.mi355_cfm_euler_sample_tiled(h, C.c_void_p(x.data_ptr()), 3, None, 0, 0, None, ts, 3, None, None, B2, C.c_void_p(ws.data_ptr()), need,
                                            stream, C.byref(p))
        assert rc < 0 and word in L.mi355_last_error().decode() and "cfm_euler_sample_tiled" in L.mi355_last_error().decode(), (bad, rc)
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    # Python: the pairs that have no tiled entry point, each named
    t = dict(stride=STRIDE)
    for kw, word in ((dict(guidance_scale=2.0), "guidance_scale"), (dict(cache_interval=2), "cache_interval"), (dict(cond_drift=True), "cond_drift"),
                     (dict(cache_schedule=[1, 0]), "cache_schedule")):
        with pytest.raises(NotImplementedError, match=f"tiling together with {word}"):
            eng.cfm_euler(x, [0.0, 0.5, 1.0], tiling=t, **kw)
    from image_diffusion.sde_diffusion import DDPM

    tables = DDPM(25).host_tables()
    for kw, word in ((dict(guidance_scale=2.0), "guidance_scale"), (dict(cache_interval=2), "cache_interval")):
        with pytest.raises(NotImplementedError, match=f"tiling together with {word}"):
            eng.ddpm_sample(x, tables, mode=_lib.DDPM_PRIOR, tiling=t, **kw)
    with pytest.raises(MI355BackendError, match="canvas_h"):
        eng.cfm_euler(torch.zeros(1, 3, 12, 40, device=DEV), [0.0, 1.0], tiling=t)
    # without tiling a mismatched size is still the ValueError it was
    with pytest.raises(ValueError, match="expected 16x16 images"):
        eng.cfm_euler(x, [0.0, 1.0])
    with pytest.raises(ValueError, match="expected 16x16 images"):
        eng.forward(x, 0.1)
    assert torch.equal(x, before)
    eng.check()
