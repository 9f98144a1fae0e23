"""GPU: the multistep samplers - the DPM-Solver++ step kernels against fp64 from their fp32 inputs (the budget proven on the CPU in
tests/test_multistep_cpu.py) and their bit-exact identities; the DPM-Solver++ samplers (fused loop and generic host loop, orders 1 and 2, prior /
amortized / guided) against the fp64 restatement (tests/multistep_ref.py) driving the CPU oracle U-Net; the Adams-Bashforth CFM samplers
(UNetEngine.cfm_ab, one library call) against the fp64 restatement on the oracle net, against the host class and through compute_fid; the
refusals that need a handle; launch counts.

Tolerances: DDPM samplers the project's bound rtol 2e-3 / atol 1e-3 (tests/test_gpu_unet.py SAMPLER_TOL); fused against generic 1e-4, 1e-4 (1 + 2|w|)
when guided (tests/test_gpu_cfg.py); CFM samplers rtol 5e-4 / atol 1e-4, library call against host loop 1e-4 (tests/test_gpu_rk.py).  Sampler-level
chains have every r_i >= 0.3 (asserted): a chain with tiny r amplifies the net's fp32 noise by 1 + 1 / (2 r) and belongs to the op tests only.
Tiny nets at 16x16, B = 3, K = 7 steps (and the unrespaced DDPM(25)).  Observed on an MI355X: DESIGN.md section 8.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mi355.synth import randn, synth_state_dict
from oracle import unet_ref
from tests import multistep_ref as M
from tests.test_ddpm_respace_cpu import EPS32
from tests.test_gpu_ddpm_respace import _banded, _bits, _report, _unband
from tests.test_multistep_cpu import R_DPMPP, coefficient_cases, dpmpp_budget, dpmpp_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STOL = dict(rtol=2e-3, atol=1e-3)
FP32 = dict(rtol=5e-4, atol=1e-4)
B, S = 3, 16
_CACHE = {}


# ---- 1. the step kernels against fp64 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,off", [(105, 0), (768, 0), (768, 1)])
def test_step_ops_vs_fp64(n, off):
    """mi355_dpmpp_step and mi355_dpmpp_cfg_step on NaN-banded buffers, 16-byte aligned and one float off: x inside (r + 1) 2^-24 M, the kept
    D inside its three roundings, two runs bit-equal, guard bands untouched.  Coefficients: DDPM(100).respace(STEPS7), orders 1 and 2."""
    from mi355.ops import default_ops as ops

    worst = dict(plain=0.0, guided=0.0)
    for k, order, a, b, cx, c0, c1 in coefficient_cases():
        x, eps, hist = dpmpp_inputs(n, a, b, 100 * k + n)
        tx, te, th = (torch.from_numpy(v) for v in (x, eps, hist))
        eu = randn(8100 + k, n)
        w = 1.75
        eg = (eu.to(DEV) + (te.to(DEV) - eu.to(DEV)) * w).cpu()      # u + w (c - u) in fp32, each operation rounded: the guided step's eps
        for guided in (False, True):
            e_in = eg.numpy() if guided else eps
            with np.errstate(invalid="ignore"):
                want, wantD, bound = dpmpp_budget(x, e_in, hist, a, b, cx, c0, c1)
                pre_mag = np.abs(float(np.float32(a)) * x.astype(np.float64)) + np.abs(float(np.float32(b)) * e_in.astype(np.float64))
            runs = []
            for _ in range(2):
                (bh, vh) = _banded(th, off)
                if guided:
                    (bx, vx2), (_, ve2) = _banded(torch.cat((tx, tx + 3.0)), off), _banded(torch.cat((te, eu)), off)
                    ops.dpmpp_cfg_step_(vx2.view(2, n), ve2.view(2, n), vh.view(1, n), w, a, b, cx, c0, c1)
                    torch.cuda.synchronize()
                    both = _unband(bx, 2 * n, off)
                    assert torch.equal(_bits(both[:n]), _bits(both[n:])), "the two halves differ"
                    runs.append((both[:n].clone(), _unband(bh, n, off)))
                else:
                    (bx, vx), (_, ve) = _banded(tx, off), _banded(te, off)
                    assert vx.data_ptr() % 16 == 4 * off
                    ops.dpmpp_step_(vx, ve, vh, a, b, cx, c0, c1)
                    torch.cuda.synchronize()
                    runs.append((_unband(bx, n, off), _unband(bh, n, off)))
            assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1])), "two runs differ"
            got, gotD = runs[0][0].double().numpy(), runs[0][1].double().numpy()
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and nan.sum() == 1 and np.array_equal(np.isnan(gotD), nan)
            key = "guided" if guided else "plain"
            worst[key] = max(worst[key], float((np.abs(got - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max()))
            assert (np.abs(gotD - wantD)[~nan] <= 4 * EPS32 * pre_mag[~nan]).all(), (k, order, guided)
    print(f"n = {n}, off = {off}: max err / budget (r = {R_DPMPP}): dpmpp_step {worst['plain']:.3f}, dpmpp_cfg_step {worst['guided']:.3f}")
    assert worst["plain"] <= 1.0 and worst["guided"] <= 1.0


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("Bn,img", [(3, (1, 5, 7)), (4, (3, 8, 8))])
def test_step_ops_identities_bit_exact(Bn, img, per_image):
    """c1 == 0 keeps a NaN-filled history out of the state (and still stores D); the guided step is the plain one on a torch-computed
    u + w (c - u), scalar and per-image w; hist = None keeps nothing; n = 0 does nothing."""
    from mi355._lib import MI355BackendError
    from mi355.ops import default_ops as ops

    x = randn(8301, Bn, *img).to(DEV)
    eps2 = randn(8302, 2 * Bn, *img).to(DEV)
    hist = (randn(8303, Bn, *img) * 0.5).to(DEV)
    co = (1.8, 1.5, 0.7, 0.9)     # c_recip, c_recipm1, cx, c0
    e1 = eps2[:Bn].contiguous()
    # c1 == 0: a NaN history is never read, and it leaves as D
    hn = torch.full_like(x, float("nan"))
    a = ops.dpmpp_step_(x.clone(), e1, hn, *co, 0.0)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(hn).all())
    assert torch.equal(hn, (1.8 * x - 1.5 * e1).clamp(-1, 1))
    assert torch.equal(a, ops.dpmpp_step_(x.clone(), e1, None, *co, 0.0))
    h2 = hist.clone()
    b = ops.dpmpp_step_(x.clone(), e1, h2, *co, -0.4)
    assert torch.equal(h2, hn) and not torch.equal(a, b)
    assert torch.equal(b, (0.7 * x + 0.9 * hn) + (-0.4) * hist)       # the kernel's operation order, in eager torch
    # guided == plain on the combined eps
    w = torch.tensor([0.5 + 0.75 * i for i in range(Bn)], device=DEV) if per_image else 1.75
    wv = w.reshape(-1, *([1] * len(img))) if per_image else w
    eg = (eps2[Bn:] + (eps2[:Bn] - eps2[Bn:]) * wv).contiguous()
    for c1 in (0.0, -0.4):
        hp, hg = hist.clone(), hist.clone()
        exp = ops.dpmpp_step_(x.clone(), eg, hp, *co, c1)
        x2 = torch.cat((x, x + 5.0))   # the second half is never read
        ops.dpmpp_cfg_step_(x2, eps2, hg, w, *co, c1)
        assert torch.equal(x2[:Bn], exp) and torch.equal(x2[Bn:], exp) and torch.equal(hg, hp), c1
    with pytest.raises(ValueError, match="hist"):
        ops.dpmpp_step_(x.clone(), e1, None, *co, 0.5)
    with pytest.raises(MI355BackendError, match="per-image"):
        from mi355 import _lib
        p = C.c_void_p(x.data_ptr())
        _lib.check(_lib.lib().mi355_dpmpp_cfg_step(p, p, None, 1.0, p, 7, 1.0, 1.0, 0.5, 0.5, 0.0, 8, None), "mi355_dpmpp_cfg_step")
    e = torch.empty(0, *img, device=DEV)
    ops.dpmpp_step_(e, e, e, *co, 0.3)
    ops.dpmpp_cfg_step_(e, e, e, 2.0, *co, 0.3)
    torch.cuda.synchronize()


# ---- nets, inputs ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets():
    from tests.test_gpu_unet import _tiny

    return {1: _tiny(1, 1, 1001, "fp32"), 2: _tiny(2, 1, 1002, "fp32")}   # in_channels -> (cfg, net, sd)


def _inputs():
    xT = randn(8601, B, 1, S, S)
    cond = (randn(8602, B, 1, S, S) * 0.5).clamp(-1, 1)
    cond[:, :, 4:10, 5:11] = -2.0
    return xT, cond


def _chains():
    from image_diffusion.sde_diffusion import DDPM

    if "chains" not in _CACHE:
        d = DDPM(100)
        _CACHE["chains"] = {"logsnr7of100": d.respace(d.logsnr_steps(7)), "25": DDPM(25)}
    return _CACHE["chains"]


def _ref_eps(nets, cin, ddpm):
    cfg, _, sd = nets[cin]
    return lambda net_in, k: unet_ref.unet_forward(sd, cfg, net_in.float(), torch.full((net_in.shape[0],), ddpm.time(k), dtype=torch.float32))


def _dpm_ref(nets, chain, mode, order):
    """The fp64 restatement over the oracle net, computed once and shared (never modified)."""
    key = ("dpm", chain, mode, order)
    if key not in _CACHE:
        r = _chains()[chain]
        xT, cond = _inputs()
        acp = r.alphas_cumprod.numpy()
        if mode == "prior":
            _CACHE[key] = M.dpmpp_sample(_ref_eps(nets, 1, r), acp, order, xT)
        else:
            _CACHE[key] = M.dpmpp_sample(_ref_eps(nets, 2, r), acp, order, xT, cond=cond, amortized=True, none_value=-2.0,
                                         w=2.0 if mode == "guided" else None)
    return _CACHE[key]


# ---- 2. the DPM-Solver++ samplers against the restatement -------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("mode", ["prior", "amortized", "guided"])
@pytest.mark.parametrize("chain", ["logsnr7of100", "25"])
def test_dpm_solver_samplers_vs_restatement(nets, chain, mode, order):
    from image_diffusion import sampling
    from image_diffusion.likelihoods import InPainting

    r = _chains()[chain]
    K = r.Ns
    ratios = M.step_ratios(r.alphas_cumprod.numpy())
    assert ratios.min() >= 0.3, (chain, ratios.min())
    lik = InPainting(patch_size=6, pad_value=-2)
    xT, cond = _inputs()
    cin = 1 if mode == "prior" else 2
    w = 2.0 if mode == "guided" else None
    net = nets[cin][1]
    ref, n_eval = _dpm_ref(nets, chain, mode, order)
    assert n_eval == K * (2 if w is not None else 1)
    fast = sampling.make_eps_model(net, r)
    asked = []
    generic = lambda xi, i: asked.append(int(i[0])) or fast(xi, i)   # noqa: E731  (untagged: the host loop over the step ops)
    args = (xT.to(DEV),) if mode == "prior" else (xT.to(DEV), cond.to(DEV))
    got = sampling.get_dpm_solver_sample_fn(fast, r, lik, guidance_scale=w, order=order)(*args).cpu()
    gen = sampling.get_dpm_solver_sample_fn(generic, r, lik, guidance_scale=w, order=order)(*args).cpu()
    assert asked == [i for i in reversed(range(K)) for _ in range(2 if w is not None else 1)]
    e1 = _report(f"{chain} {mode} order {order}: fused vs fp64 restatement", got, ref)
    e2 = _report(f"{chain} {mode} order {order}: fused vs generic", got, gen)
    assert (ref - xT.double()).abs().max() > 1e-2 and float(got.abs().max()) <= 1.0
    torch.testing.assert_close(got.double(), ref, **STOL)
    gb = 1e-4 * (1 + 2 * abs(w)) if w is not None else 1e-4
    torch.testing.assert_close(got, gen, rtol=gb, atol=gb)
    if order == 1:   # the deterministic DDIM step, written with other coefficients
        ddim = sampling.get_ddim_sample_fn(fast, r, lik, guidance_scale=w)(*args).cpu()
        _report(f"{chain} {mode}: order 1 vs get_ddim_sample_fn", got, ddim)
        torch.testing.assert_close(got, ddim, rtol=gb, atol=gb)
    else:            # and the second order is another sampler: it moved the result beyond the tolerance
        d12 = float((ref - _dpm_ref(nets, chain, mode, 1)[0]).abs().max())
        print(f"{chain} {mode}: order 2 vs order 1 restatements differ by {d12:.3e}")
    assert np.isfinite(e1) and np.isfinite(e2)
    net.engine(DEV).check()


def test_multistep_launch_counts_and_determinism(nets):
    """mi355_unet_get_stats after a multistep call: the launches of the last evaluation (those of the DDIM loop's) plus ONE step launch; the
    call is deterministic; a guided per-image scale equal to the scalar gives the scalar's bits; guided slices carry their rows."""
    from mi355 import _lib

    r = _chains()["logsnr7of100"]
    T = r.host_tables()
    coefs = r.dpm_solver_coefs(2)
    xT, cond = (t.to(DEV) for t in _inputs())
    sched = dict(timesteps=r.timesteps, train_steps=r.base_Ns)
    for cin, kw in ((1, {}), (2, dict(cond=cond)), (2, dict(cond=cond, guidance_scale=2.0))):
        eng = nets[cin][1].engine(DEV)
        eng.ddpm_sample(xT.clone(), T, mode=_lib.DDIM, **kw, **sched)
        n0 = eng.stats(B)["launches"]
        a = eng.ddpm_multistep(xT.clone(), T, coefs, **kw, **sched)
        n1 = eng.stats(B)["launches"]
        b = eng.ddpm_multistep(xT.clone(), T, coefs, **kw, **sched)
        print(f"in_channels {cin} {sorted(kw)}: launches of the last evaluation {n0}, of the last multistep step {n1}")
        assert n1 == n0 + 1 and n0 > 0
        assert torch.equal(_bits(a), _bits(b)) and (a - xT).abs().max() > 1e-2
        eng.check()
    eng = nets[2][1].engine(DEV)
    a = eng.ddpm_multistep(xT.clone(), T, coefs, cond=cond, guidance_scale=2.0, **sched)
    b = eng.ddpm_multistep(xT.clone(), T, coefs, cond=cond, guidance_scale=torch.full((B,), 2.0, device=DEV), **sched)
    assert torch.equal(_bits(a), _bits(b))
    eng.max_batch_override = 4      # cfg_batch() = 2: slices of 2 and 1 images
    try:
        c = eng.ddpm_multistep(xT.clone(), T, coefs, cond=cond, guidance_scale=2.0, **sched)
    finally:
        eng.max_batch_override = None
    torch.testing.assert_close(c, a, rtol=5e-4, atol=5e-4)   # a slice's kernels may sum in another order: the fused-vs-generic bound, 1e-4 (1 + 2|w|)
    eng.check()


def test_multistep_refusals_with_a_handle(nets):
    """Refusals that need a handle: an error code and a text each, nothing launched, the stream and the handle stay usable."""
    from mi355 import _lib

    L = _lib.lib()
    r = _chains()["logsnr7of100"]
    K = r.Ns
    T = r.host_tables()
    xT, cond = (t.to(DEV) for t in _inputs())
    x = xT.clone()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    cs = [c.contiguous() for c in r.dpm_solver_coefs(2)]
    steps = (C.c_int32 * K)(*r.timesteps)

    def ms(c1=None, train=r.base_Ns):
        m = _lib.MultistepScheduleC()
        m.steps, m.train_steps = C.cast(steps, ip), train
        m.cx, m.c0 = C.cast(cs[0].data_ptr(), fp), C.cast(cs[1].data_ptr(), fp)
        m.c1 = C.cast((cs[2] if c1 is None else c1).data_ptr(), fp)
        return m

    def call(eng, m, mode=_lib.DDIM, guided=False, channels=1, cp=None, short=0, batch=B):
        tb, keep = eng._ddpm_tables(T)
        opt = _lib.DDPMOptionsC(mode, 0, 0.1, 1e-5, 1.0, 1.0, 1, -2.0, -2.0, int(cp is None), 0)
        xp = C.c_void_p(x.data_ptr())
        ws, wsb = eng._workspace_sized("mi355_ddpm_multistep_workspace_bytes", B, int(guided))
        if guided:
            return L.mi355_ddpm_multistep_cfg_sample(eng.handle, xp, channels, cp, None, 0, 2.0, None, C.byref(tb), C.byref(opt), C.byref(m), batch, ws,
                                                     wsb - short, eng._stream())
        return L.mi355_ddpm_multistep_sample(eng.handle, xp, channels, cp, C.byref(tb), C.byref(opt), C.byref(m), batch, ws, wsb - short, eng._stream())

    e1, e2 = nets[1][1].engine(DEV), nets[2][1].engine(DEV)
    cp = C.c_void_p(cond.data_ptr())
    # the workspace amount: the unscheduled entry point's, rounded up to 256, plus one state rounded up to 256
    state = (B * S * S * 4 + 255) // 256 * 256
    assert L.mi355_ddpm_multistep_workspace_bytes(e1.handle, B, 0) == (L.mi355_unet_workspace_bytes(e1.handle, B) + 255) // 256 * 256 + state
    assert L.mi355_ddpm_multistep_workspace_bytes(e2.handle, B, 1) == (L.mi355_ddpm_cfg_workspace_bytes(e2.handle, B) + 255) // 256 * 256 + state
    assert L.mi355_ddpm_multistep_workspace_bytes(e1.handle, 0, 0) < 0
    bad_c1 = cs[2].clone()
    bad_c1[K - 1] = 0.25
    cases = [(e1, dict(m=ms(c1=bad_c1)), -1, b"c1[K-1]"), (e1, dict(m=ms(), mode=_lib.DDPM_PRIOR), -1, b"MI355_DDIM"),
             (e1, dict(m=ms(train=0)), -1, b"train_steps"), (e1, dict(m=ms(), short=1), -2, b"workspace too small"),
             (e1, dict(m=ms(), channels=2), -2, b"channel count"), (e1, dict(m=ms(), batch=0), -1, b"bad argument"),
             (e2, dict(m=ms(), guided=True), -1, b"nothing to guide"), (e2, dict(m=ms(), guided=True, cp=cp, short=1), -2, b"workspace too small"),
             (e1, dict(m=ms(), guided=True, cp=cp), -2, b"2C-input"), (e2, dict(m=ms(c1=bad_c1), guided=True, cp=cp), -1, b"c1[K-1]")]
    for eng, kw, rc, msg in cases:
        got = call(eng, **kw)
        assert got == rc and msg in L.mi355_last_error(), (kw, got, L.mi355_last_error())
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(xT))   # nothing was launched
    for eng in (e1, e2):
        eng.check()
    assert call(e1, ms()) == 0                 # a correct call follows
    torch.cuda.synchronize()
    e1.check()
    want = e1.ddpm_multistep(xT.clone(), T, cs, timesteps=r.timesteps, train_steps=r.base_Ns)
    assert torch.equal(_bits(x), _bits(want))
    x.copy_(xT)
    assert call(e2, ms(), guided=True, cp=cp) == 0
    torch.cuda.synchronize()
    e2.check()
    assert not torch.equal(x, xT)
    with pytest.raises(ValueError, match="one entry per step"):
        e1.ddpm_multistep(xT.clone(), T, [c[:3] for c in cs])
    with pytest.raises(ValueError, match="go together"):
        e1.ddpm_multistep(xT.clone(), T, cs, timesteps=r.timesteps)
    with pytest.raises(NotImplementedError):
        e1.ddpm_multistep(xT.clone(), T, cs, y=torch.zeros(B, dtype=torch.long, device=DEV))


# ---- 3. Adams-Bashforth ---------------------------------------------------------------------------------------------------------------------

GRID = [0.0, 0.05, 0.07, 0.3, 0.5, 0.85, 1.0]      # 6 intervals, non-uniform
ORDER = {"ab2": 2, "ab3": 3, "ab4": 4}


def _x0(seed=8901):
    return randn(seed, B, 1, S, S)


def _ab_ref(nets, method):
    key = ("ab", method)
    if key not in _CACHE:
        cfg, _, sd = nets[1]
        f = lambda t, x: unet_ref.unet_forward(sd, cfg, x.float(), torch.full((x.shape[0],), t, dtype=torch.float32))   # noqa: E731
        _CACHE[key] = M.ab_integrate(f, _x0(), GRID, ORDER[method])
    return _CACHE[key]


@pytest.mark.parametrize("method", ["ab2", "ab3", "ab4"])
def test_cfm_ab_vs_restatement(nets, method):
    """UNetEngine.cfm_ab (one library call) against the fp64 restatement over the oracle net: the final state and every trajectory entry;
    traj[0] the input and traj[-1] the state exactly; the uint8 output the quantised state; the evaluations counted through the launches of
    the last step; the library call against the host class; a single time; fewer steps than the start needs."""
    from mi355.ode import AB_START, AdamsBashforth, resolve_tableau
    from mi355.ops import default_ops as ops

    q = ORDER[method]
    ref = _ab_ref(nets, method)
    refs = {m: _ab_ref(nets, m)[-1] for m in ORDER}
    tol = FP32["atol"] + FP32["rtol"] * max(float(v.abs().max()) for v in refs.values())
    for m in ORDER:      # the comparison can tell the orders apart (6.5 x the tolerance between ab3 and ab4 on the CPU oracle)
        assert m == method or float((refs[m] - refs[method]).abs().max()) >= 5 * tol, (m, method)
    eng = nets[1][1].engine(DEV)
    x0 = _x0()
    x = x0.to(DEV)
    xr, traj, u8 = eng.cfm_ab(x, GRID, method, keep_traj=True, want_u8=True)
    assert xr is x
    n_last = eng.stats(B)["launches"]
    _report(f"cfm_ab {method} final", x.cpu(), ref[-1])
    torch.testing.assert_close(x.cpu().double(), ref[-1], **FP32)
    assert traj.shape == (len(GRID),) + tuple(x0.shape) and torch.equal(traj[0].cpu(), x0) and torch.equal(traj[-1], x)
    for k in range(len(GRID)):
        torch.testing.assert_close(traj[k].cpu().double(), ref[k], **FP32)
    assert u8.dtype == torch.uint8 and torch.equal(u8, ops.quantize_u8(x))
    x2 = x0.to(DEV)      # without the optional outputs: the same state
    _, t2, u2 = eng.cfm_ab(x2, GRID, method)
    assert t2 is None and u2 is None and torch.equal(x2, x)
    # the last step is a multistep step: one evaluation (mi355_cfm_rk_sample reports its last evaluation's launches) and one stage launch
    eng.cfm_rk(x0.to(DEV), GRID, "euler")
    n_eval = eng.stats(B)["launches"]
    print(f"{method}: launches of the last step {n_last}; of one evaluation {n_eval}")
    assert n_last == n_eval + 1 and n_eval > 0
    # the host class: the same rule, one forward and one rk_stage launch per evaluation
    sol = AdamsBashforth(lambda t, y: [eng.forward(y[0], float(t))], method)
    host = torch.stack([x0.to(DEV)] + [s[0] for s in sol.integrate_times([x0.to(DEV)], GRID)])
    stages = len(resolve_tableau(AB_START[method])[1])
    assert sol.nfe == M.ab_evaluations(len(GRID) - 1, q, stages)
    _report(f"cfm_ab {method} library call vs host class", traj.cpu(), host.cpu())
    torch.testing.assert_close(traj, host, rtol=1e-4, atol=1e-4)
    # n_t == 1: no step; traj[0] and the bytes are still written
    xs = x0.to(DEV)
    _, tr1, u1 = eng.cfm_ab(xs, [0.3], method, keep_traj=True, want_u8=True)
    assert torch.equal(xs.cpu(), x0) and tr1.shape[0] == 1 and torch.equal(tr1[0].cpu(), x0) and torch.equal(u1, ops.quantize_u8(xs))
    # n_steps < order - 1 (one step; for ab2 it is the one start step): the start method's steps, bit for bit
    xa, xb = x0.to(DEV), x0.to(DEV)
    eng.cfm_ab(xa, GRID[:2], method, want_u8=True)
    eng.cfm_rk(xb, GRID[:2], AB_START[method])
    assert torch.equal(_bits(xa), _bits(xb))
    if q > 2:
        xa, xb = x0.to(DEV), x0.to(DEV)
        eng.cfm_ab(xa, GRID[:q], method)
        eng.cfm_rk(xb, GRID[:q], AB_START[method])
        assert torch.equal(_bits(xa), _bits(xb))
    torch.cuda.synchronize()
    eng.check()


@pytest.mark.parametrize("method", ["ab2", "ab4"])
def test_cfm_ab_guided_and_labelled(nets, method):
    """The guided form against a two-call host loop (the host class over the guided forward) and against the restatement over the oracle's
    two evaluations; the labelled form against the restatement on a class-conditional tiny net; slices."""
    from mi355.ode import AdamsBashforth
    from tests.test_classcond_cpu import ClassCondConfig, classcond_forward
    from tests.test_gpu_classcond import _model

    q = ORDER[method]
    cfg, net, sd = nets[2]
    eng = net.engine(DEV)
    x0, cond = _x0(8902), _inputs()[1]
    w = 2.0
    x = x0.to(DEV)
    _, traj, u8 = eng.cfm_ab(x, GRID, method, cond=cond.to(DEV), guidance_scale=w, none_value=-2.0, keep_traj=True, want_u8=True)
    sol = AdamsBashforth(lambda t, y: [eng.forward(y[0], float(t), cond=cond.to(DEV), guidance_scale=w, none_value=-2.0)], method)
    host = torch.stack([x0.to(DEV)] + [s[0] for s in sol.integrate_times([x0.to(DEV)], GRID)])
    _report(f"guided cfm_ab {method} vs two-call host loop", traj.cpu(), host.cpu())
    torch.testing.assert_close(traj, host, rtol=1e-4 * (1 + 2 * w), atol=1e-4 * (1 + 2 * w))
    assert torch.equal(traj[0].cpu(), x0) and torch.equal(traj[-1], x)

    def f(t, xx):
        tt = torch.full((xx.shape[0],), t, dtype=torch.float32)
        vc = unet_ref.unet_forward(sd, cfg, torch.cat((xx.float(), cond), dim=1), tt).double()
        vu = unet_ref.unet_forward(sd, cfg, torch.cat((xx.float(), torch.full_like(cond, -2.0)), dim=1), tt).double()
        return vu + w * (vc - vu)

    ref = M.ab_integrate(f, x0, GRID, q)
    _report(f"guided cfm_ab {method} vs fp64 restatement", x.cpu(), ref[-1])
    gt = dict(rtol=FP32["rtol"] * (1 + 2 * w), atol=FP32["atol"] * (1 + 2 * w))   # the guided field carries (1 + 2|w|) of each evaluation's error
    torch.testing.assert_close(x.cpu().double(), ref[-1], **gt)
    # slices: cfg_batch() = 2
    eng.max_batch_override = 4
    try:
        xs = x0.to(DEV)
        _, trs, _ = eng.cfm_ab(xs, GRID, method, cond=cond.to(DEV), guidance_scale=w, keep_traj=True)
    finally:
        eng.max_batch_override = None
    torch.testing.assert_close(trs, traj, rtol=1e-5, atol=1e-6)
    eng.check()
    # labels
    base = nets[1][0]
    ccfg = ClassCondConfig(**{k: getattr(base, k) for k in base.__dataclass_fields__}, num_classes=5)
    if "cc" not in _CACHE:
        _CACHE["cc"] = _model(ccfg, 8903, "fp32")
    m, csd = _CACHE["cc"]
    y = torch.tensor([3, 0, 4])
    fl = lambda t, xx: classcond_forward(csd, ccfg, xx.float(), torch.full((xx.shape[0],), t, dtype=torch.float32), y)   # noqa: E731
    refl = M.ab_integrate(fl, x0, GRID, q)
    xl = x0.to(DEV)
    m.engine(DEV).cfm_ab(xl, GRID, method, y=y.to(DEV))
    _report(f"labelled cfm_ab {method} vs fp64 restatement", xl.cpu(), refl[-1])
    torch.testing.assert_close(xl.cpu().double(), refl[-1], **FP32)
    xg = x0.to(DEV)   # labels and guidance: w = 1 is the conditional model up to the rounding of u + (c - u)
    m.engine(DEV).cfm_ab(xg, GRID, method, y=y.to(DEV), guidance_scale=1.0, null_label=1)
    torch.testing.assert_close(xg.cpu().double(), refl[-1], **FP32)
    m.engine(DEV).check()


def test_neural_ode_and_make_gen_1_img_ab2():
    """NeuralODE(wrapper, solver="ab3") is one library call and agrees with the host class; compute_fid's --integration_method ab2: uint8
    [B, 3, 32, 32], the same seed gives the same bytes, the next call a fresh batch, and not Euler's images."""
    import compute_fid
    from image_diffusion.unet import param_shapes
    from mi355.ode import AdamsBashforth
    from tests.test_gpu_sde import _wrappers
    from torchcfm_compat import NeuralODE

    (m,) = _wrappers(False, (8951,))
    x0 = randn(8952, 5, 1, 28, 28).to(DEV)
    ts = torch.tensor([0.0, 0.2, 0.25, 0.6, 1.0])
    fast = NeuralODE(m, solver="ab3").trajectory(x0, ts)
    eng = m.engine(DEV)
    sol = AdamsBashforth(lambda t, y: [eng.forward(y[0], float(t))], "ab3")
    host = torch.stack([x0] + [s[0] for s in sol.integrate_times([x0], ts.tolist())])
    assert sol.nfe == 2 * 2 + 2 and fast.shape == host.shape == (5, 5, 1, 28, 28)
    torch.testing.assert_close(fast, host, rtol=1e-4, atol=1e-4)
    assert torch.equal(fast[0], x0) and (fast[-1] - x0).abs().max() > 1e-2
    plain = NeuralODE(lambda t, x: m(t, x), solver="ab3").trajectory(x0, ts)   # a callable that is no wrapper: the host class
    torch.testing.assert_close(plain, host, rtol=1e-4, atol=1e-4)

    net = compute_fid.build_model(128, DEV, precision="fp32")
    net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
    Bf, steps = 40, 8
    gen = compute_fid.make_gen_1_img(net, batch_size_fid=Bf, integration_steps=steps, integration_method="ab2", device=DEV, seed=11)
    img = gen(None)
    assert img.dtype == torch.uint8 and img.shape == (Bf, 3, 32, 32) and img.device.type == "cuda"
    again = compute_fid.make_gen_1_img(net, batch_size_fid=Bf, integration_steps=steps, integration_method="ab2", device=DEV, seed=11)(None)
    assert torch.equal(img, again)
    assert not torch.equal(gen(None), img)
    euler = compute_fid.make_gen_1_img(net, batch_size_fid=Bf, integration_steps=steps, integration_method="euler", device=DEV, seed=11)(None)
    assert not torch.equal(euler, img)
    x = compute_fid.draw_x0_shard(Bf, 11, 0, torch.device(DEV))
    _, _, want = net.engine(DEV).cfm_ab(x, torch.linspace(0, 1, steps + 1).tolist(), "ab2", want_u8=True)
    assert torch.equal(img, want)


def test_cfm_ab_refusals_with_a_handle(nets):
    """Argument errors of mi355_cfm_ab_sample / mi355_cfm_ab_cfg_sample that need a handle: an error code and a text each, nothing launched;
    the handle stays usable."""
    from mi355.ode import ab_weights, resolve_tableau

    eng = nets[1][1].engine(DEV)
    L = eng.L
    x0 = _x0().to(DEV)
    x = x0.clone()
    a, b, c = resolve_tableau("midpoint")
    fa, fb, fc = (C.c_float * 4)(*[v for r in a for v in r]), (C.c_float * 2)(*b), (C.c_float * 2)(*c)
    ts = (C.c_float * len(GRID))(*GRID)
    wt = ab_weights(GRID, 3).contiguous()
    wp = C.cast(wt.data_ptr(), C.POINTER(C.c_float))
    ws, wsb = eng._workspace_sized("mi355_cfm_ab_workspace_bytes", B, 3, 2, 0)
    need = L.mi355_cfm_ab_workspace_bytes(eng.handle, B, 3, 2, 0)
    base = L.mi355_unet_workspace_bytes(eng.handle, B)
    state = (B * S * S * 4 + 255) // 256 * 256
    assert need == (base + 255) // 256 * 256 + (3 + 1 + 1) * state          # the ring, the start's second stage, the stage state
    assert L.mi355_cfm_ab_workspace_bytes(eng.handle, B, 3, 2, 0) == L.mi355_cfm_rk_workspace_bytes(eng.handle, B, 4)
    for bad in ((B, 1, 2, 0), (B, 5, 2, 0), (B, 3, 0, 0), (B, 3, 5, 0), (0, 3, 2, 0)):
        assert L.mi355_cfm_ab_workspace_bytes(eng.handle, *bad) < 0
    lab = torch.zeros(B, dtype=torch.int32, device=DEV)
    xp = C.c_void_p(x.data_ptr())

    def call(labels=None, xc=1, bytes_=wsb, order=3, guided=False, batch=B):
        if guided:
            return L.mi355_cfm_ab_cfg_sample(eng.handle, xp, xc, None, 0, -2.0, labels, 0, 2.0, None, ts, len(GRID), order, wp, 2, fa, fb, fc, None, None,
                                             batch, ws, bytes_, eng._stream())
        return L.mi355_cfm_ab_sample(eng.handle, xp, xc, None, 0, labels, ts, len(GRID), order, wp, 2, fa, fb, fc, None, None, batch, ws, bytes_,
                                     eng._stream())

    for kw, rc, text in ((dict(bytes_=need - 1), -2, b"workspace too small"), (dict(labels=C.c_void_p(lab.data_ptr())), -1, b"num_classes"),
                         (dict(xc=2), -2, b"channel count"), (dict(order=5), -1, b"order"), (dict(batch=0), -1, b"bad argument"),
                         (dict(guided=True), -1, b"nothing to guide")):
        got = call(**kw)
        assert got == rc and text in L.mi355_last_error(), (kw, got, L.mi355_last_error())
    torch.cuda.synchronize()
    assert torch.equal(x, x0)      # nothing ran
    eng.check()
    assert call() == 0             # the handle is still usable: a valid call, and the same numbers as through the engine
    torch.cuda.synchronize()
    eng.check()
    want = x0.clone()
    eng.cfm_ab(want, GRID, "ab3")
    assert torch.equal(_bits(x), _bits(want))
    with pytest.raises(NotImplementedError):
        eng.cfm_ab(x, GRID, "ab5")
    with pytest.raises(ValueError, match="sum_j a_ij"):     # a first stage off t_k is no tableau of resolve_tableau's at all
        eng.cfm_ab(x, GRID, "ab2", start=([[], [1.0]], [0.5, 0.5], [0.5, 1.0]))
    with pytest.raises(ValueError, match="monotone"):
        eng.cfm_ab(x, [0.0, 0.5, 0.5, 1.0], "ab2")
    with pytest.raises(ValueError, match="num_classes"):
        eng.cfm_ab(x, GRID, "ab2", y=lab)
