"""GPU: training-free in-painting / super-resolution with an unconditional flow net - the low-resolution consistency seed
(mi355_lowres_seed) against fp64, the one-call sampler (mi355_cfm_recon_sample) against the CPU restatement tests/flow_guidance_ref.py
under torch.autograd, its exact invariants, get_flow_conditional_sample_fn and the DDPM ReconstructionGuidance with LowResolution.

Seed bound, elementwise: |got - fp64| <= (r + 1) * eps32 * M, r the fp32 roundings on the element's path and M the sum of the absolute
values of its terms (test_gpu_rk.py's stage bound); the fp64 value is computed from the fp32 inputs and the fp32 tap weights.  Counted
from the kernels' expressions (csrc/backward.hip), a contracted product-and-sum being one rounding fewer:
  resid = h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11) - y,  v = clip(c_recip x - c_recipm1 eps):   3 (pre: two products, one difference)
          + 1 (w v) + 1 (inner sum) + 1 (h ..) + 1 (outer sum) + 1 (- y)                                              r = 8
  g     = k ((wy wx) resid), k = 2 / per rounded on the host:  8 + 1 (k) + 1 (wy wx) + 1 (w resid) + 1 (k ..)         r = 12
  g_eps = -c_recipm1 g, g_x = c_recip g:                       12 + 1                                                 r = 13
  loss  = mean(resid^2): the square doubles the residual's relative error (2 * 8), then the reduction - ceil(per / 256) serial terms per
          thread, 6 shuffle levels, 3 partial sums, the division and the conversion to fp32 (the sums are fp64: counted all the same)
                                                                                                r = 16 + ceil(per / 256) + 11
The clip rule is a comparison: an element whose pre is within rounding of -1 or +1 could fall on either side in fp32 and fp64, so the
inputs are built with no such element (those few are set to x = eps = 0), apart from the planted ones whose pre is exactly -1 or +1.

Sampler tolerances: fp32 the project's bound for its other guided sampler (rtol 2e-3, atol 1e-3, tests/test_gpu_guidance.py), losses rtol
2e-3.  bf16: per image against the fp32 CPU restatement, relative rms error and max|err| / max|ref|, bounds at 3x the worst image
measured on the MI355X (the margin of _check_bf16_images / SYNTH_BF16), the measured values next to the bounds (RECON_BF16)."""
import ctypes as C
import math

import pytest
import torch

from mi355.synth import rand_uniform, randn
from oracle import cfm_ref, ddpm_ref, unet_ref
from tests import flow_guidance_ref as fref
from tests.test_classcond_cpu import classcond_forward, load_case
from tests.test_gpu_guidance import VJP_SYNTH, _build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = float(torch.finfo(torch.float32).eps)
STOL = dict(rtol=2e-3, atol=1e-3)
GUARD = 64   # floats of NaN on both sides of every output (256 bytes: the views keep the buffer's alignment)


# ---- 1. lowres_seed against fp64 ----------------------------------------------------------------------------------------------------

def _seed_inputs(B, Cc, H, W, h, w, cr, cm, idx):
    """x, eps scaled so that about a third of pre = cr x - cm eps leaves [-1, 1]; no element within rounding of the clip edges; planted: pre
    exactly +1 and -1 (x = +-1 / cr when that is exact, eps = 0) and one NaN at a tap of low-res pixel (0, 0) of image 0."""
    a = 0.9674 / math.sqrt(cr * cr + cm * cm)        # P(|N(0, 1)| > 0.9674) = 1 / 3
    x, eps = a * randn(5000 + idx, B, Cc, H, W), a * randn(5100 + idx, B, Cc, H, W)
    y = rand_uniform(5200 + idx, -1, 1, B, Cc, h, w)
    crf, cmf = float(torch.tensor(cr, dtype=torch.float32)), float(torch.tensor(cm, dtype=torch.float32))
    pre = crf * x.double() - cmf * eps.double()
    near = ((pre.abs() - 1).abs() < 8 * EPS32 * ((crf * x.double()).abs() + (cmf * eps.double()).abs() + 1))
    x[near], eps[near] = 0.0, 0.0
    n = x.numel()
    xf, ef = x.view(-1), eps.view(-1)
    xf[n // 3], ef[n // 3] = 1.0, 0.0
    xf[n // 2], ef[n // 2] = -1.0, 0.0
    x[0, 0, int(fref.axis_taps(h, H)[0][0]), int(fref.axis_taps(w, W)[0][0])] = float("nan")
    return x, eps, y


def _banded(t, off):
    """A copy of t on the device as a view into a NaN-filled buffer, GUARD floats of band on both sides, `off` floats off the band's grid."""
    buf = torch.full((t.numel() + 2 * GUARD + 4,), float("nan"), device=DEV)
    view = buf[GUARD + off:GUARD + off + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _bits(t):
    return t.contiguous().view(torch.int32)


SEED_SHAPES = [(2, 3, 16, 16, 4, 4, 0), (2, 3, 16, 16, 8, 8, 0), (3, 1, 12, 10, 4, 5, 0), (1, 3, 64, 64, 16, 16, 0), (2, 3, 16, 16, 1, 1, 0),
               (2, 3, 16, 16, 16, 16, 0), (2, 3, 16, 16, 4, 4, 1)]   # last: every tensor a view 4 bytes off the 16-byte grid


@pytest.mark.parametrize("coef", [(1.0, -0.6), (1.7, 1.37)], ids=["flow", "ddpm"])
@pytest.mark.parametrize("B,Cc,H,W,h,w,off", SEED_SHAPES)
def test_lowres_seed_vs_fp64(B, Cc, H, W, h, w, off, coef):
    from mi355 import _lib

    L = _lib.lib()
    cr, cm = coef
    x, eps, y = _seed_inputs(B, Cc, H, W, h, w, cr, cm, SEED_SHAPES.index((B, Cc, H, W, h, w, off)))
    ref = fref.lowres_seed_ref64(x, eps, y, cr, cm)
    ok = ~torch.isnan(ref["pre"])
    frac = float(((ref["pre"][ok] < -1) | (ref["pre"][ok] > 1)).double().mean())
    print(f"clipped fraction {frac:.3f}")
    assert 0.10 <= frac <= 0.60
    assert bool((ref["pre"] == 1).any()) == (cr == 1.0) and bool((ref["pre"] == -1).any()) == (cr == 1.0)   # the planted +-1 (flow coefficients)
    (_, xd), (_, ed), (_, yd) = _banded(x, off), _banded(eps, off), _banded(y, off)
    runs = []
    for _ in range(2):
        out = {k: _banded(torch.full(s, float("nan")), off) for k, s in
               (("resid", y.shape), ("g_eps", x.shape), ("g_x", x.shape), ("loss", (B,)))}
        ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        assert (xd.data_ptr() % 16 == 4 * off) and (out["g_x"][1].data_ptr() % 16 == 4 * off)
        rc = L.mi355_lowres_seed(ptr(xd), ptr(ed), ptr(yd), cr, cm, B, Cc, H, W, h, w, ptr(out["resid"][1]), ptr(out["g_eps"][1]),
                                 ptr(out["g_x"][1]), ptr(out["loss"][1]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.mi355_last_error()
        torch.cuda.synchronize()
        runs.append({k: b.cpu() for k, (b, _) in out.items()})
    for k in runs[0]:
        assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), f"{k}: two runs differ"
    per = Cc * h * w
    r_of = dict(resid=8, g_eps=13, g_x=13, loss=16 + math.ceil(per / 256) + 11)
    M_of = dict(resid=ref["M_resid"], g_eps=ref["M_g_eps"], g_x=ref["M_g_x"], loss=ref["M_loss"])
    for k, buf in runs[0].items():
        want = ref[k]
        n = want.numel()
        lo, got, hi = buf[:GUARD + off], buf[GUARD + off:GUARD + off + n].view(want.shape).double(), buf[GUARD + off + n:]
        assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all()), f"{k}: a guard band was written"
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), f"{k}: NaN pattern"
        err = (got - want).abs()[~nan]
        bound = ((r_of[k] + 1) * EPS32 * M_of[k])[~nan]
        ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        print(f"   {k}: max err / bound {ratio:.3f} (r = {r_of[k]}), {int(nan.sum())} NaN")
        assert bool((err <= bound).all()), k
    assert bool(torch.isnan(ref["loss"][0])) and not bool(torch.isnan(ref["loss"][1:]).any())
    clipped = ~((ref["pre"] >= -1) & (ref["pre"] <= 1))
    got_gx = runs[0]["g_x"][GUARD + off:GUARD + off + x.numel()].view(x.shape)
    assert not bool(got_gx[clipped].any())   # exactly zero wherever pre is outside [-1, 1] or NaN


def test_lowres_seed_op_and_refusal():
    from mi355._lib import MI355BackendError
    from mi355.ops import default_ops as ops

    x, eps, y = (t.to(DEV) for t in _seed_inputs(2, 3, 16, 16, 8, 8, 1.0, -0.6, 90))
    g_eps, g_x, loss = ops.lowres_seed(x, eps, y, 1.0, -0.6)
    ref = fref.lowres_seed_ref64(x.cpu(), eps.cpu(), y.cpu(), 1.0, -0.6)
    torch.testing.assert_close(g_x.cpu().double(), ref["g_x"], rtol=1e-5, atol=1e-7, equal_nan=True)
    torch.testing.assert_close(g_eps.cpu().double(), ref["g_eps"], rtol=1e-5, atol=1e-7, equal_nan=True)
    torch.testing.assert_close(loss.cpu().double(), ref["loss"], rtol=1e-5, atol=1e-7, equal_nan=True)
    with pytest.raises(MI355BackendError, match="integer factors"):
        ops.lowres_seed(x, eps, torch.zeros(2, 3, 5, 8, device=DEV), 1.0, -0.6)


# ---- 2. / 3. the sampler against the CPU restatement ------------------------------------------------------------------------------------

B, TS = 3, [float(v) for v in torch.linspace(0, 1, 7)]
# name -> (net, mode, gamma, replace, final_paste)
CASES = {
    "paint": ("t16_heads2", 0, 0.5, None, False),
    "paint_coupled": ("t16_heads2", 0, 0.5, "coupled", True),
    "hyper": ("t16_heads2", 1, 0.5 * 3 * 16 * 16, None, False),
    "lowres": ("t16_heads2", 2, 200.0, None, False),
    "ch96_paint": ("ch96_192", 0, 0.5, None, False),
    "labels_lowres": ("classcond", 2, 200.0, None, False),
}
LABELS = torch.tensor([4, 1, 0])


def _net(name, golden, precision="fp32"):
    """-> (model on the device, state dict, cfg, CPU forward(x, t[B]), labels or None)"""
    if name == "classcond":
        from tests.test_gpu_classcond import _model

        g, cfg = load_case(golden, "tiny_film_updown_neworder")
        net, sd = _model(cfg, int(g["seed"]), precision)
        return net, sd, cfg, (lambda x, t: classcond_forward(sd, cfg, x, t, LABELS)), LABELS
    cfg = VJP_SYNTH[name]
    net, sd = _build(cfg, 2002 if name == "t16_heads2" else 2000, precision)
    return net, sd, cfg, (lambda x, t: unet_ref.unet_forward_diff(sd, cfg, x, t)), None


def _inputs(mode):
    x0 = randn(11, B, 3, 16, 16)
    img = rand_uniform(12, -1, 1, B, 3, 16, 16)
    if mode == 0:
        y = img.clone()
        y[:, :, 5:11, 4:10] = -2.0
    elif mode == 1:
        y = cfm_ref.hyperresolution_condition(img, 4, 4)
    else:
        y = fref.lowres_D(img, (4, 4))
    return x0, y


_REF = {}


def _reference(case, golden):
    """The CPU restatement of a case, computed once and shared by the fp32 and the bf16 test."""
    if case not in _REF:
        name, mode, gamma, replace, fp = CASES[case]
        _, sd, cfg, fwd, _ = _net(name, golden)
        x0, y = _inputs(mode)
        scales = [float(torch.tensor(gamma, dtype=torch.float32))] * (len(TS) - 1)
        _REF[case] = fref.flow_recon_ref(sd, cfg, x0, TS, y, mode, scales, replace, fp, forward=fwd)
    return _REF[case]


def _run_case(case, golden, precision):
    name, mode, gamma, replace, fp = CASES[case]
    net, _, _, _, labels = _net(name, golden, precision)
    x0, y = _inputs(mode)
    eng = net.engine(DEV, differentiable=True)
    assert eng.precision == precision
    x = x0.to(DEV).clone()
    _, traj, _, loss = eng.cfm_recon(x, TS, y.to(DEV), mode, scales=[gamma] * (len(TS) - 1), replace=replace, final_paste=fp, keep_traj=True,
                                     return_loss=mode == 2, y_labels=None if labels is None else labels.to(DEV))
    eng.check()
    return x.cpu(), traj.cpu(), None if loss is None else loss.cpu()


@pytest.mark.parametrize("case", list(CASES))
def test_sampler_fp32_vs_reference(case, golden):
    ref = _reference(case, golden)
    x, traj, loss = _run_case(case, golden, "fp32")
    err = (x - ref["x"]).abs()
    print(f"{case} fp32: max|err| {float(err.max()):.3e}, max|ref| {float(ref['x'].abs().max()):.3f}, "
          f"moved by guidance / replacement: rms(x - x0) {float((ref['x'] - ref['traj'][0]).pow(2).mean().sqrt()):.3f}")
    torch.testing.assert_close(x, ref["x"], **STOL)
    torch.testing.assert_close(traj, ref["traj"], **STOL)
    if loss is not None:
        print(f"   losses: ref {ref['losses'][:, 0].tolist()}")
        torch.testing.assert_close(loss, ref["losses"], rtol=2e-3, atol=0)


# per image vs the fp32 CPU restatement, (relative rms, max|err| / max|ref|): 3x the worst image measured on the MI355X, which was
# paint (6.69e-3, 4.82e-2), paint_coupled (5.51e-3, 1.03e-2), hyper (3.47e-3, 2.09e-2), lowres (3.16e-3, 1.17e-2),
# ch96_paint (5.14e-2, 2.84e-1), labels_lowres (7.04e-3, 4.48e-2).  The max figures are single pixels (plausibly ones whose x1_hat sits at a clip edge, where
# the whole guidance term switches under bf16 rounding; not analysed further), the rms figures the image.
RECON_BF16 = {
    "paint": (0.020, 0.145), "paint_coupled": (0.0165, 0.031), "hyper": (0.0104, 0.063), "lowres": (0.0095, 0.035), "ch96_paint": (0.154, 0.85),
    "labels_lowres": (0.021, 0.135),
}


@pytest.mark.parametrize("case", list(CASES))
def test_sampler_bf16_vs_reference(case, golden):
    ref = _reference(case, golden)["x"]
    x, _, _ = _run_case(case, golden, "bf16")
    assert torch.isfinite(x).all()
    dims = (1, 2, 3)
    rms = (x - ref).pow(2).mean(dim=dims).sqrt() / ref.pow(2).mean(dim=dims).sqrt()
    mx = (x - ref).abs().amax(dim=dims) / ref.abs().amax(dim=dims)
    rb, mb = RECON_BF16[case]
    print(f"{case} bf16: worst per-image relative rms {float(rms.max()):.3e} (bound {rb}), worst per-image max|err|/max|ref| {float(mx.max()):.3e} "
          f"(bound {mb})")
    assert float(rms.max()) < rb, rms.tolist()
    assert float(mx.max()) < mb, mx.tolist()


# ---- 4. exact invariants --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def t16():
    net, _ = _build(VJP_SYNTH["t16_heads2"], 2002)
    return net


def test_final_paste_returns_the_measurement(t16):
    x0, y = _inputs(0)
    yd = y.to(DEV)
    known = y != -2.0
    for replace, kw in (("coupled", {}), ("fresh", dict(seed=5))):
        for eng, scales in ((t16.engine(DEV), None), (t16.engine(DEV, differentiable=True), [0.5] * 6)):
            x = x0.to(DEV).clone()
            _, traj, u8, _ = eng.cfm_recon(x, TS, yd, 0, scales=scales, replace=replace, final_paste=True, keep_traj=True, want_u8=True, **kw)
            assert TS[-1] == 1.0 and torch.equal(_bits(x.cpu()[known]), _bits(y[known])), replace
            assert not torch.equal(x.cpu()[~known], x0[~known])
            assert torch.equal(traj[-1], x) and torch.equal(traj[0].cpu(), x0)   # the last slot and the bytes are the pasted state's
            from mi355.ops import default_ops as ops

            assert torch.equal(u8, ops.quantize_u8(x))


def test_unguided_is_the_euler_sampler(t16):
    from mi355.ops import default_ops as ops

    x0, y = _inputs(0)
    for eng in (t16.engine(DEV), t16.engine(DEV, differentiable=True)):
        xa, xb, xc = (x0.to(DEV).clone() for _ in range(3))
        _, ta, ua, _ = eng.cfm_recon(xa, TS, None, 0, keep_traj=True, want_u8=True)
        n_plain = eng.stats(B)["launches"]
        _, tb, ub = eng.cfm_rk(xb, TS, method="euler", keep_traj=True, want_u8=True)
        assert torch.equal(xa, xb) and torch.equal(ta, tb) and torch.equal(ua, ub)
        assert torch.equal(ua, ops.quantize_u8(xa))
        # (e) all scales 0.0: the unguided result, and no backward pass (the step's launch count is the unguided step's)
        if eng.differentiable:
            eng.cfm_recon(xc, TS, y.to(DEV), 0, scales=[0.0] * 6)
            assert torch.equal(xc, xa) and eng.stats(B)["launches"] == n_plain
            xg = x0.to(DEV).clone()
            eng.cfm_recon(xg, TS, y.to(DEV), 0, scales=[0.0] * 5 + [0.5])
            n_guided = eng.stats(B)["launches"]
            print(f"launches of the last step: unguided {n_plain}, guided {n_guided}")
            assert n_guided > n_plain + 2 and not torch.equal(xg, xa)


def test_fresh_replacement_injected_draws_are_the_philox_path(t16):
    from mi355.ops import default_ops as ops

    x0, y = _inputs(0)
    eng = t16.engine(DEV)
    n = x0.numel()
    assert n % 4 == 0   # n_al == n
    seed = 1234567
    draws = torch.stack([ops.randn(tuple(x0.shape), DEV, seed, k * n) for k in range(len(TS))])
    for fp in (False, True):
        xa, xb = x0.to(DEV).clone(), x0.to(DEV).clone()
        eng.cfm_recon(xa, TS, y.to(DEV), 0, replace="fresh", final_paste=fp, seed=seed)
        eng.cfm_recon(xb, TS, y.to(DEV), 0, replace="fresh", final_paste=fp, noise=draws)
        assert torch.equal(xa, xb), fp
    xc = x0.to(DEV).clone()
    eng.cfm_recon(xc, TS, y.to(DEV), 0, replace="fresh", seed=seed + 1)
    assert not torch.equal(xc, xa)


def test_trajectory_slots_and_image_bytes(t16):
    from mi355.ops import default_ops as ops

    x0, y = _inputs(2)
    eng = t16.engine(DEV, differentiable=True)
    x = x0.to(DEV).clone()
    _, traj, u8, loss = eng.cfm_recon(x, TS, y.to(DEV), 2, scales=[200.0, 0.0, 200.0, 200.0, 0.0, 200.0], keep_traj=True, want_u8=True,
                                      return_loss=True)
    assert torch.equal(traj[0].cpu(), x0) and torch.equal(traj[-1], x) and torch.equal(u8, ops.quantize_u8(x))
    assert torch.isnan(loss[[1, 4]]).all() and torch.isfinite(loss[[0, 2, 3, 5]]).all()   # rows of unguided steps: NaN
    for k in (1, 3, 4):   # traj[k] is the state after step k - 1: the same call over the first k steps ends there
        xk = x0.to(DEV).clone()
        eng.cfm_recon(xk, TS[:k + 1], y.to(DEV), 2, scales=[200.0, 0.0, 200.0, 200.0, 0.0, 200.0][:k])
        assert torch.equal(xk, traj[k]), k


def test_library_refusals_on_a_handle(t16):
    from mi355._lib import MI355BackendError

    x0, y = _inputs(0)
    eng, deng = t16.engine(DEV), t16.engine(DEV, differentiable=True)
    L = eng.L
    # a non-zero scale on a handle without the differentiable plan: the unet_vjp error code, before any launch (x untouched)
    ts = (C.c_float * 3)(0.0, 0.5, 1.0)
    sc = (C.c_float * 2)(0.5, 0.5)
    x = x0.to(DEV).clone()
    yd = y.to(DEV)
    ws, _ = deng._workspace_sized("mi355_cfm_recon_workspace_bytes", B, 4, 4)   # the larger of the two handles' needs
    wsb = L.mi355_cfm_recon_workspace_bytes(deng.handle, B, 0, 0)

    def call(handle=eng.handle, scales=sc, mode=0, hl=0, wl=0, ws=ws, wsb=wsb, labels=None, loss=None):
        return L.mi355_cfm_recon_sample(handle, C.c_void_p(x.data_ptr()), 3, labels, ts, 3, C.c_void_p(yd.data_ptr()), mode, -2.0, hl, wl, scales, 0, 0,
                                        None, 0, None, None, loss, B, ws, wsb, None)

    assert call() == -4 and b"differentiable" in L.mi355_last_error()
    assert call(handle=deng.handle, wsb=wsb - 1) == -2                                       # short workspace
    assert call(handle=deng.handle, ws=C.c_void_p(ws.value + 16)) == -1                      # misaligned workspace
    assert call(handle=deng.handle, mode=2, hl=5, wl=4) == -4 and b"integer factors" in L.mi355_last_error()
    assert call(handle=deng.handle, labels=C.c_void_p(x.data_ptr())) == -1 and b"num_classes" in L.mi355_last_error()
    assert call(handle=deng.handle, loss=C.c_void_p(x.data_ptr())) == -1
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), x0)
    need = L.mi355_cfm_recon_workspace_bytes(eng.handle, B, 4, 4)
    base = L.mi355_unet_workspace_bytes(eng.handle, B)
    state = B * 3 * 16 * 16 * 4
    assert need == (base + 255) // 256 * 256 + 4 * state + (B * 3 * 4 * 4 * 4 + 255) // 256 * 256
    with pytest.raises(MI355BackendError, match="differentiable"):
        eng.cfm_recon(x, TS, yd, 0, scales=[0.5] * 6)
    # an amortized (2C-input) net is not for this sampler
    cfg2 = unet_ref.UNetConfig(16, 6, 32, 3, 1, (4,), channel_mult=(1, 2, 2), num_heads=2)
    net2, _ = _build(cfg2, 2003)
    e2 = net2.engine(DEV)
    ws2, wsb2 = e2._workspace_sized("mi355_cfm_recon_workspace_bytes", B, 0, 0)
    assert call(handle=e2.handle, scales=None, ws=ws2, wsb=wsb2) == -2 and b"amortized" in L.mi355_last_error()


# ---- 5. get_flow_conditional_sample_fn ------------------------------------------------------------------------------------------------

def test_flow_sample_fn_is_the_manual_composition(t16):
    from flow_sampling import get_flow_conditional_sample_fn
    from image_diffusion.conditioning import FlowReconstructionGuidance, FlowReplacement
    from image_diffusion.likelihoods import InPainting, LowResolution

    x0, y = _inputs(0)
    cond = FlowReconstructionGuidance(0.5, 0.5, "one_minus_t", "coupled")
    got = get_flow_conditional_sample_fn(t16, cond, InPainting(6, -2.0), TS)(x0.to(DEV), y.to(DEV))
    x = x0.to(DEV).clone()
    t16.engine(DEV, differentiable=True).cfm_recon(x, TS[:4], y.to(DEV), 0, scales=cond.scales(TS[:3]), replace="coupled", final_paste=False)
    t16.engine(DEV).cfm_euler(x, TS[3:])
    assert torch.equal(got, x) and not torch.equal(got.cpu(), x0)
    # the whole span guided: the last paste is on; replacement alone runs on the plain engine
    full = get_flow_conditional_sample_fn(t16, FlowReplacement(1.0, "coupled"), InPainting(6, -2.0), TS)(x0.to(DEV), y.to(DEV)).cpu()
    known = y != -2.0
    assert torch.equal(full[known], y[known])
    # LowResolution: mode 2 through the factory, against the restatement
    x0, ylow = _inputs(2)
    lr = get_flow_conditional_sample_fn(t16, FlowReconstructionGuidance(200.0, 1.0, "constant", None), LowResolution(4, 4), TS)(x0.to(DEV), ylow.to(DEV))
    torch.testing.assert_close(lr.cpu(), _reference("lowres", None)["x"], **STOL)


def test_flow_sample_fn_slices_a_large_batch(t16):
    from flow_sampling import get_flow_conditional_sample_fn
    from image_diffusion.conditioning import FlowReconstructionGuidance
    from image_diffusion.likelihoods import InPainting

    x0 = randn(21, 5, 3, 16, 16)
    y = rand_uniform(22, -1, 1, 5, 3, 16, 16)
    y[:, :, 5:11, 4:10] = -2.0
    sample = get_flow_conditional_sample_fn(t16, FlowReconstructionGuidance(0.5, 0.5, "constant", "coupled"), InPainting(6, -2.0), TS)
    whole = sample(x0.to(DEV), y.to(DEV)).cpu()
    engines = (t16.engine(DEV), t16.engine(DEV, differentiable=True))
    try:
        for e in engines:
            e.max_batch_override = 2
        sliced = sample(x0.to(DEV), y.to(DEV)).cpu()
    finally:
        for e in engines:
            e.max_batch_override = None
    print(f"sliced vs whole: max|diff| {float((sliced - whole).abs().max()):.3e}")
    torch.testing.assert_close(sliced, whole, **STOL)


# ---- 6. DDPM ReconstructionGuidance with the low-resolution likelihood ------------------------------------------------------------------

def test_ddpm_reconstruction_guidance_with_low_resolution():
    from image_diffusion import sampling
    from image_diffusion.conditioning import ReconstructionGuidance
    from image_diffusion.likelihoods import LowResolution
    from image_diffusion.sde_diffusion import DDPM

    Ns, gamma, sf = 25, 100.0, 0.2
    cfg = unet_ref.UNetConfig(16, 1, 32, 1, 1, (2,), channel_mult=(1, 2), num_heads=2)
    net, sd = _build(cfg, 2004)
    xT = randn(31, 3, 1, 16, 16)
    lik = LowResolution(4, 4)
    ylow = lik.sample(rand_uniform(32, -1, 1, 3, 1, 16, 16))
    draws = [randn(700 + j, *xT.shape) for j in range(Ns)]
    it = iter(draws)
    eps_ref = ddpm_ref.make_eps_model(lambda x, t: unet_ref.unet_forward_diff(sd, cfg, x, t), Ns)
    ref = fref.ddpm_lowres_guidance_ref(eps_ref, Ns, xT, ylow, lambda shape: next(it), gamma=gamma, start_fraction=sf)
    it = iter(draws)
    plain = fref.ddpm_lowres_guidance_ref(eps_ref, Ns, xT, ylow, lambda shape: next(it), gamma=0.0, start_fraction=sf)
    ddpm = DDPM(Ns)
    with sampling.injected_noise(draws):
        got = sampling.get_conditional_sample_fn(sampling.make_eps_model(net, ddpm), ddpm, ReconstructionGuidance(gamma, sf, "before", 0, 0.1), lik)(
            xT.to(DEV), ylow.to(DEV)).cpu()
    print(f"ddpm lowres guidance: max|err| {float((got - ref).abs().max()):.3e}; the guidance moved the result by "
          f"max {float((ref - plain).abs().max()):.3e}")
    assert float((ref - plain).abs().max()) > 10 * STOL["atol"]   # the guidance term matters in the result
    torch.testing.assert_close(got, ref, **STOL)
