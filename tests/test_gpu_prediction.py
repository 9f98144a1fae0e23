"""GPU: x0- and v-prediction DDPM nets (mi355_ddpm_pred_sample, mi355_ddpm_vlb_pred, mi355_pred_step, mi355_pred_shape_stats, mi355_vlb_terms_pred;
DDPM.with_prediction, DDPM.with_fixed_variance).
  1. the eps kind through every new op and through mi355_ddpm_pred_sample is the existing op / entry point, bit for bit, with the same launch count;
  2. mi355_pred_step against fp64 inside the budget tests/test_prediction_cpu.py derives: every step kind x prediction kind x {plain, guided w,
     guided w_dev} x {clipped, shaped} x {contiguous, strided} that exists (shaping rows need the contiguous read; the corrector has no guided and
     no shaped form; the learned-variance step is strided and unshaped);
  3. the statistics op of the x0 and v kinds against the existing op fed the algebraically equivalent eps;
  4. the loops on a respaced chain, x0 and v kinds: fused vs the host loop, vs the fp64 restatement driven by the same fp32 network, and away from
     the eps-kind result on the same net;
  5. the bound per kind against fp64, the mse target of the kind, fixed large against fixed small;
  6. the public path is one library call per batch, and the refusals that need a handle.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mi355.synth import randn
from tests import prediction_ref as PR
from tests import vlb_ref as VR
from tests.test_ddpm_respace_cpu import EPS32
from tests.test_gpu_ddpm_respace import _banded, _bits, _report, _unband
from tests.test_prediction_cpu import B, PERS, PREDS, R_PRE, STEP_KINDS, pred_budget, pred_cases, pred_operands
from tests.test_vlb_cpu import vlb_cases, vlb_operands
from tests.test_x0_shaping_cpu import rows_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STOL = dict(rtol=2e-3, atol=1e-3)      # SAMPLER_TOL: the fused samplers against an fp64 restatement (tests/test_gpu_ddpm_respace.py)
S = 16
W = 4.0
V_GAIN = 3.0
_CACHE = {}
FORMS = {"ddpm": ((False, False), (False, True), (True, False)), "ddim": ((False, False), (False, True), (True, False)),
         "ddim_eta": ((False, False), (False, True), (True, False)), "dpmpp": ((False, False), (False, True), (True, False)),
         "corrector": ((False, False), (False, True)), "ddpm_lv": ((False, True),)}      # (shaped, strided)


def _step_args(kind, case):
    """case["c"][kind] -> (c_recip, c_recipm1, a, b, c, keywords) of Ops.pred_step_."""
    c = case["c"][kind]
    kw = dict(sa=case["sa"], sb=case["sb"])
    if kind == "ddpm":
        return c[0], c[1], c[2], c[3], 0.0, dict(kw, sigma=c[4])
    if kind == "ddpm_lv":
        return c[0], c[1], c[2], c[3], 0.0, dict(kw, min_log=c[4], max_log=c[5])
    if kind in ("ddim", "ddim_eta"):
        return c[0], c[1], c[2], 0.0, 0.0, dict(kw, sigma=c[3])
    return c[0], c[1], c[2], c[3], c[4], kw      # dpmpp: cx, c0, c1; corrector: rsm1, dt, delta


def _mix32(oc, ou, w, per):
    """cfg_mix in fp32 numpy: the difference, the product and the sum each rounded."""
    wv = np.repeat(w.numpy().astype(np.float32), per) if isinstance(w, torch.Tensor) else np.float32(w)
    d = (oc - ou).astype(np.float32)
    return (ou + (wv * d).astype(np.float32)).astype(np.float32)


def _run_step(ops, kind, pred, case, x, o, ou, z, hist, var, rows, w, per, strided):
    """One pred_step_ launch on banded operands -> (x_new [n], hist_new [n] or None); asserts the two halves of a guided step equal."""
    n = B * per
    guided = w is not None
    lead = 2 * B if guided else B
    first = torch.from_numpy(np.concatenate((o, ou)) if guided else o).view(lead, 1, per)
    out = first
    if strided:     # the second channel: the variance channel where the step reads it (the conditional half's), NaN everywhere else
        second = torch.full((lead, 1, per), float("nan"))
        if var is not None:
            second[:B] = torch.from_numpy(var).view(B, 1, per)
        out = torch.cat((first, second), dim=1)
    tx = torch.from_numpy(x).view(B, 1, per)
    bx, vx = _banded(torch.cat((tx, tx + 3.0)) if guided else tx, 1)
    assert vx.data_ptr() % 16 == 4
    _, vo = _banded(out, 2 if strided else 3)
    bh, vh = _banded(torch.from_numpy(hist).view(B, 1, per), 1) if hist is not None else (None, None)
    zt = torch.from_numpy(z).to(DEV).view(B, 1, per) if z is not None else None
    cr, crm1, a, b, c, kw = _step_args(kind, case)
    ops.pred_step_(kind, pred, vx, vo, cr, crm1, a, b, c, z=zt, hist=vh, w=(w.to(DEV) if isinstance(w, torch.Tensor) else w),
                   shape=None if rows is None else torch.from_numpy(np.stack(rows, 1)).to(DEV).contiguous(), **kw)
    torch.cuda.synchronize()
    both = _unband(bx, vx.numel(), 1)
    if guided:
        assert torch.equal(_bits(both[:n]), _bits(both[n:])), "the two halves differ"
    return both[:n].clone(), (_unband(bh, n, 1).clone() if bh is not None else None)


# ---- 1. the eps kind is today's bits -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", PERS)
def test_eps_kind_ops_are_the_existing_ops(per):
    from mi355.ops import default_ops as ops

    n = B * per
    wt = torch.tensor([1.75, 0.5, 3.0], device=DEV)
    seen = set()
    for j, case in enumerate(pred_cases()):
        for kind in STEP_KINDS:
            for shaped, strided in FORMS[kind]:
                x, o, z, hist, var = pred_operands(kind, "eps", per, case, 500 * j + per, shaped)
                ou = randn(9900 + j, n).numpy()
                rows = rows_for(n, per, 9 * j + n) if shaped else None
                for w in ((None,) if kind == "corrector" else (None, 2.5, wt)):
                    guided = w is not None
                    lead = 2 * B if guided else B
                    e = torch.from_numpy(np.concatenate((o, ou)) if guided else o).view(lead, 1, per)
                    second = torch.full((lead, 1, per), float("nan"))
                    if var is not None:
                        second[:B] = torch.from_numpy(var).view(B, 1, per)
                    wide = torch.cat((e, second), dim=1).to(DEV)
                    rt = None if rows is None else torch.from_numpy(np.stack(rows, 1)).to(DEV).contiguous()
                    cr, crm1, a, b, c, kw = _step_args(kind, case)
                    res = {}
                    for form in ("new", "old"):
                        tx = torch.from_numpy(x).view(B, 1, per)
                        bx, vx = _banded(torch.cat((tx, tx + 3.0)) if guided else tx, 1)
                        bh, vh = _banded(torch.from_numpy(hist).view(B, 1, per), 1) if hist is not None else (None, None)
                        zt = torch.from_numpy(z).to(DEV).view(B, 1, per) if z is not None else None
                        src = wide if strided else e.to(DEV).contiguous()
                        if form == "new":
                            ops.pred_step_(kind, "eps", vx, src, cr, crm1, a, b, c, z=zt, hist=vh, w=w, shape=rt, **kw)
                        elif kind == "ddpm_lv":
                            ops.ddpm_lv_step_(vx, src, zt, cr, crm1, a, b, kw["min_log"], kw["max_log"], w=w)
                        elif strided:
                            ops.strided_step_(kind, vx, src, cr, crm1, a, b, c, sigma=kw.get("sigma", 0.0), z=zt, hist=vh, w=w)
                        elif kind == "corrector":
                            ops.corrector_step_(vx, src, zt, cr, crm1, a, b, c)
                        else:
                            ops.x0_shaped_step_(kind, vx, src, rt, cr, crm1, a, b, c, sigma=kw.get("sigma", 0.0), z=zt, hist=vh, w=w)
                        torch.cuda.synchronize()
                        res[form] = (_unband(bx, vx.numel(), 1).clone(), _unband(bh, n, 1).clone() if bh is not None else None)
                    assert torch.equal(_bits(res["new"][0]), _bits(res["old"][0])), (kind, shaped, strided, guided)
                    assert not torch.equal(_bits(res["new"][0][:n]), _bits(torch.from_numpy(x))), "the step did nothing"
                    if hist is not None:
                        assert torch.equal(_bits(res["new"][1]), _bits(res["old"][1]))
                    seen.add((kind, shaped, strided, guided, isinstance(w, torch.Tensor)))
    assert len(seen) == 4 * 3 * 3 + 2 + 3
    # the statistics op and the bound's terms op
    case = pred_cases()[1]
    cr, crm1 = case["c"]["ddpm"][:2]
    x, o, _, _, _ = pred_operands("ddpm", "eps", per, case, 77 + per, True)
    ou = randn(9950, n).numpy()
    xt = torch.from_numpy(x).view(B, 1, per).to(DEV)
    for w in (None, 2.5, wt):
        e = torch.from_numpy(np.concatenate((o, ou)) if w is not None else o).view(-1, 1, per).to(DEV)
        sh = (0.9, 2.0, 0.7 if w is not None else 0.0)
        new = ops.pred_shape_stats("eps", xt, e, cr, crm1, sh, sa=case["sa"], sb=case["sb"], w=w, detail=True)
        old = ops.x0_shape_stats(xt, e, cr, crm1, sh, w=w, detail=True)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(new, old))
    k, sc = vlb_cases()[2]
    x0, xk, eps, v, z = vlb_operands(per, sc, 700 + per)
    kwsc = {name: sc[name] for name in VR.SCALARS}
    for learned in (False, True):
        out = torch.stack((torch.from_numpy(eps), torch.from_numpy(v)), 1).to(DEV)
        args = [torch.from_numpy(a).view(B, 1, per).to(DEV) for a in (x0, xk)]
        zt = torch.from_numpy(z).view(B, 1, per).to(DEV)
        new = ops.vlb_terms(*args, out, z=zt, k_is_zero=False, learned=learned, prediction="eps", sa=sc["sa"], sb=sc["sb"], **kwsc)
        old = ops.vlb_terms(*args, out, z=zt, k_is_zero=False, learned=learned, **kwsc)
        assert torch.equal(_bits(new), _bits(old))


# ---- nets, inputs ---------------------------------------------------------------------------------------------------------------------------------------

def _lv_net(in_ch, Cs, seed):
    from tests.test_gpu_unet import _tiny

    cfg, net, sd = _tiny(in_ch, 2 * Cs, seed, "fp32")
    sd = {k: t.clone() for k, t in sd.items()}
    sd["out.2.weight"][Cs:] *= V_GAIN
    sd["out.2.bias"][Cs:] *= V_GAIN
    net.load_state_dict(sd)
    return net.to(DEV)


@pytest.fixture(scope="module")
def nets():
    from tests.test_gpu_unet import _tiny

    return {(1, 1): _tiny(1, 1, 1001, "fp32")[1], (2, 1): _tiny(2, 1, 1002, "fp32")[1], (1, 2): _lv_net(1, 1, 1011), (2, 2): _lv_net(2, 1, 1012)}


def _inputs():
    xT = randn(8801, B, 1, S, S)
    cond = (randn(8802, B, 1, S, S) * 0.5).clamp(-1, 1)
    cond[:, :, 4:10, 5:11] = -2.0
    return xT, cond


def _chain():
    from image_diffusion.sde_diffusion import DDPM

    if "chain" not in _CACHE:
        d = DDPM(100)
        _CACHE["chain"] = d.respace(d.logsnr_steps(7))
    return _CACHE["chain"]


def _draws(n=40):
    return randn(8901, n, B, 1, S, S)


def _net_out(net, ddpm):
    def out(net_in, k):
        t = torch.full((net_in.shape[0],), ddpm.time(k), dtype=torch.float32, device=DEV)
        return net(net_in.float().to(DEV).contiguous(), t).cpu()

    return out


@pytest.mark.parametrize("loop", ["prior", "amortized_corrector", "repaint_corrector", "guided", "guided_ddim_eta", "dpm", "dpm_guided", "shaped_guided",
                                  "shaped_dpm", "learned", "learned_guided"])
def test_eps_kind_through_the_new_entry_point_is_the_existing_one(nets, loop):
    """All six loops (plain and guided, scheduled, multistep), shaped and learned: the result bits of the loop's own entry point, and the launch
    count mi355_unet_get_stats reports after mi355_ddpm_lv_sample resp. mi355_ddpm_shaped_sample."""
    from image_diffusion.conditioning import repaint_walk
    from mi355 import _lib

    r = _chain()
    T, ml = r.host_tables(), r.max_log()
    xT, cond = (t.to(DEV) for t in _inputs())
    noise = _draws().to(DEV)
    sched = dict(timesteps=r.timesteps, train_steps=r.base_Ns)
    coefs = r.dpm_solver_coefs(2)
    shaping = (0.9, 2.0, 0.7)
    cin, cout, kw = {"prior": (1, 1, dict(mode=_lib.DDPM_PRIOR, noise=noise)),
                     "amortized_corrector": (2, 1, dict(mode=_lib.DDPM_AMORTIZED, cond=cond, noise=noise, n_corrector=1, **sched)),
                     "repaint_corrector": (1, 1, dict(mode=_lib.DDPM_REPLACEMENT, cond=cond, noise=noise, start_fraction=0.8, n_corrector=1,
                                                      walk=repaint_walk(r.Ns, 2, 2), **sched)),
                     "guided": (2, 1, dict(mode=_lib.DDPM_AMORTIZED, cond=cond, noise=noise, guidance_scale=W, n_corrector=1)),
                     "guided_ddim_eta": (2, 1, dict(mode=_lib.DDIM, cond=cond, noise=noise, guidance_scale=W, ddim_sigma=r.ddim_sigma(0.5), **sched)),
                     "dpm": (1, 1, dict(mode=_lib.DDIM, coefs=coefs, **sched)),
                     "dpm_guided": (2, 1, dict(mode=_lib.DDIM, coefs=coefs, cond=cond, guidance_scale=W, **sched)),
                     "shaped_guided": (2, 1, dict(mode=_lib.DDPM_AMORTIZED, cond=cond, noise=noise, guidance_scale=W, **sched)),
                     "shaped_dpm": (2, 1, dict(mode=_lib.DDIM, coefs=coefs, cond=cond, guidance_scale=W, **sched)),
                     "learned": (1, 2, dict(mode=_lib.DDPM_PRIOR, noise=noise, **sched)),
                     "learned_guided": (2, 2, dict(mode=_lib.DDPM_AMORTIZED, cond=cond, noise=noise, guidance_scale=W, n_corrector=1, **sched))}[loop]
    eng = nets[(cin, cout)].engine(DEV)
    if loop.startswith("shaped"):
        want = eng.ddpm_shaped(xT.clone(), T, shaping, **kw)
        n_want = eng.stats(B)["launches"]
        got = eng.ddpm_pred(xT.clone(), T, "eps", shaping=shaping, **kw)
        n_got = eng.stats(B)["launches"]
        none = eng.ddpm_pred(xT.clone(), T, None, shaping=shaping, **kw)
    elif loop.startswith("learned"):
        want = eng.ddpm_learned(xT.clone(), T, ml, **kw)
        n_want = eng.stats(B)["launches"]
        got = eng.ddpm_pred(xT.clone(), T, "eps", max_log=ml, **kw)
        n_got = eng.stats(B)["launches"]
        none = eng.ddpm_pred(xT.clone(), T, None, max_log=ml, **kw)
    else:
        own = {k: v for k, v in kw.items() if k not in ("coefs", "mode")}
        want = eng.ddpm_multistep(xT.clone(), T, coefs, **own) if loop.startswith("dpm") else eng.ddpm_sample(xT.clone(), T, **kw)
        lv = eng.ddpm_learned(xT.clone(), T, None, **kw)
        n_want = eng.stats(B)["launches"]
        assert torch.equal(_bits(lv), _bits(want))
        got = eng.ddpm_pred(xT.clone(), T, "eps", **kw)
        n_got = eng.stats(B)["launches"]
        none = eng.ddpm_sample(xT.clone(), T, prediction="eps", **kw) if not loop.startswith("dpm") else got
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(none), _bits(want)) and (want - xT).abs().max() > 1e-2
    assert n_got == n_want and n_want > 0, (n_got, n_want)
    eng.check()


# ---- 2. every step against fp64 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("pred", PREDS)
def test_pred_step_vs_fp64(per, pred):
    from mi355.ops import default_ops as ops

    n = B * per
    wt = torch.tensor([1.75, 0.5, 3.0])
    worst, seen = {}, set()
    for j, case in enumerate(pred_cases()):
        for kind in STEP_KINDS:
            for shaped, strided in FORMS[kind]:
                x, o, z, hist, var = pred_operands(kind, pred, per, case, 1000 * j + 37 * STEP_KINDS.index(kind) + per, shaped)
                ou = randn(9800 + j, n).numpy()
                rows = rows_for(n, per, 9 * j + n) if shaped else None
                for w in ((None,) if kind == "corrector" else (None, 2.5, wt)):
                    o_in = o if w is None else _mix32(o, ou, w, per)
                    with np.errstate(invalid="ignore"):
                        want, xh, bound, bound0 = pred_budget(kind, pred, x, o_in, case, z=z, hist=hist, var=var, f=None if rows is None else rows[0],
                                                              s=None if rows is None else rows[1], per=per)
                    runs = [_run_step(ops, kind, pred, case, x, o, ou, z, hist, var, rows, w, per, strided) for _ in range(2)]
                    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])), "two runs differ"
                    got = runs[0][0].double().numpy()
                    nan = np.isnan(want)
                    assert np.array_equal(np.isnan(got), nan) and nan.sum() == (1 if n >= 8 else 0), (kind, shaped, strided, "the NaN count is not as planted")
                    ratio = float((np.abs(got - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max())
                    key = kind + ("_shaped" if shaped else "") + ("_strided" if strided else "") + ("" if w is None else "_w_dev" if isinstance(w, torch.Tensor) else "_w")
                    worst[key] = max(worst.get(key, 0.0), ratio)
                    if hist is not None:      # the history is the data prediction itself
                        assert torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
                        gh = runs[0][1].double().numpy()
                        fin = np.isfinite(xh)
                        assert np.array_equal(np.isfinite(gh), fin)
                        assert (np.abs(gh - xh)[fin] <= bound0[fin]).all(), (kind, shaped, strided)
                        if pred == "x0":      # x0_pre = out: x is not read for it, the planted NaN of x does not reach the history
                            assert fin.all()
                            if not shaped:
                                assert np.array_equal(runs[0][1].numpy().view(np.uint32), np.clip(o_in, -1.0, 1.0).astype(np.float32).view(np.uint32))
                    seen.add(key)
    print(f"per = {per}, {pred}: pred_step max err / budget {({k: round(t, 3) for k, t in sorted(worst.items())})}")
    assert len(seen) == 4 * 3 * 3 + 2 + 3 and max(worst.values()) <= 1.0, worst


# ---- 3. the statistics op -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("pred", ["x0", "v"])
def test_shape_stats_of_a_kind_are_those_of_the_equivalent_eps(per, pred):
    """s is the q-quantile of |x0_pre| over the image, 1-Lipschitz in the sup norm of x0_pre: the x0_pre of the kind (r_pre roundings on its P) and the
    x0_pre of the eps op on the algebraically equivalent eps (3 roundings on P_eps, plus the rounding of that eps to fp32, c_recipm1 EPS32 |eps|)
    differ by at most the sum of their budgets; the interpolation lo + frac (hi - lo) adds 3 EPS32 s on each side."""
    from mi355.ops import default_ops as ops

    n = B * per
    worst = 0.0
    for j, case in enumerate(pred_cases()):
        cr, crm1 = (float(np.float32(v)) for v in case["c"]["ddpm"][:2])
        sa, sb = float(np.float32(case["sa"])), float(np.float32(case["sb"]))
        x, o, _, _, _ = pred_operands("ddpm", pred, per, case, 4000 * j + per, True)
        x[~np.isfinite(x)] = 0.25          # the statistics of an image with a NaN are NaN: tested by the existing op's tests
        x64, o64 = x.astype(np.float64), o.astype(np.float64)
        pre = PR.x0_pre(pred, x64, o64, cr, crm1, sa, sb)
        eps_eq = ((cr * x64 - pre) / crm1).astype(np.float32)
        xt, ot, et = (torch.from_numpy(a).view(B, 1, per).to(DEV) for a in (x, o, eps_eq))
        for q, cap in ((0.9, None), (0.995, 1.5), (1.0, None)):
            sh = (q, cap, 0.0)
            got = ops.pred_shape_stats(pred, xt, ot, cr, crm1, sh, sa=sa, sb=sb, detail=True)
            again = ops.pred_shape_stats(pred, xt, ot, cr, crm1, sh, sa=sa, sb=sb, detail=True)
            ref = ops.x0_shape_stats(xt, et, cr, crm1, sh, detail=True)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again)), "two runs differ"
            P_kind = {"x0": np.abs(o64), "v": np.abs(sa * x64) + sb * np.abs(o64)}[pred]
            e64 = eps_eq.astype(np.float64)
            P_eps = np.abs(cr * x64) + crm1 * np.abs(e64)
            tol = ((R_PRE[pred] + 1) * EPS32 * P_kind + (3 + 1) * EPS32 * P_eps + crm1 * EPS32 * np.abs(e64)).reshape(B, per).max(axis=1)
            s_raw, s_ref = got[1][:, 2].cpu().double().numpy(), ref[1][:, 2].cpu().double().numpy()
            tol = tol + 6 * EPS32 * np.abs(s_ref)
            worst = max(worst, float((np.abs(s_raw - s_ref) / tol).max()))
            assert (np.abs(s_raw - s_ref) <= tol).all(), (q, s_raw, s_ref, tol)
            lo, hi = 1.0, (cap or np.inf)
            assert (np.abs(got[0][:, 1].cpu().double().numpy() - np.clip(s_ref, lo, hi)) <= tol).all() and bool((got[0][:, 0] == 1.0).all())
            if pred == "x0":
                # fed the eps op's own fp32 x0_pre, the x0 kind selects among the same bit patterns: the rows are equal exactly
                f32 = np.float32
                pre32 = (f32(cr) * x - f32(crm1) * eps_eq).astype(np.float32)
                own = ops.pred_shape_stats("x0", xt, torch.from_numpy(pre32).view(B, 1, per).to(DEV), cr, crm1, sh, detail=True)
                assert torch.equal(_bits(own[0]), _bits(ref[0])) and torch.equal(_bits(own[1][:, 2]), _bits(ref[1][:, 2]))
                # and x is not read: a NaN-filled x gives the same rows
                blind = ops.pred_shape_stats("x0", torch.full_like(xt, float("nan")), ot, cr, crm1, sh, detail=True)
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(blind, got))
        # the rescale factor is a property of the raw outputs: the kind's op and the eps op give the same f on the same pair
        ou = randn(9700 + j, n).numpy()
        pair = torch.from_numpy(np.concatenate((o, ou))).view(2 * B, 1, per).to(DEV)
        for w in (2.5, torch.tensor([1.75, 0.5, 3.0], device=DEV)):
            a = ops.pred_shape_stats(pred, xt, pair, cr, crm1, (0.9, None, 0.7), sa=sa, sb=sb, w=w, detail=True)
            b = ops.x0_shape_stats(xt, pair, cr, crm1, (0.0, None, 0.7), w=w, detail=True)
            assert torch.equal(_bits(a[0][:, 0]), _bits(b[0][:, 0])) and torch.equal(_bits(a[1][:, :2]), _bits(b[1][:, :2]))
            # s of the guided, rescaled output: the quantile of |x0_pre(f * mix)| in fp64 from the op's own f
            f = a[0][:, 0].cpu().double().numpy()
            wv = w.cpu().double().numpy() if isinstance(w, torch.Tensor) else np.full(B, w)
            mixed = _mix32(o, ou, w.cpu() if isinstance(w, torch.Tensor) else w, per).astype(np.float64)
            fe = (np.repeat(f, per) * mixed).astype(np.float32).astype(np.float64)
            pre_g = np.abs(PR.x0_pre(pred, x64, fe, cr, crm1, sa, sb)).reshape(B, per)
            want = np.quantile(pre_g, float(np.float32(0.9)), axis=1)
            Pg = ({"x0": np.abs(fe), "v": np.abs(sa * x64) + sb * np.abs(fe)}[pred]).reshape(B, per).max(axis=1)
            assert (np.abs(a[1][:, 2].cpu().double().numpy() - want) <= (R_PRE[pred] + 1 + 6) * EPS32 * np.maximum(Pg, want)).all(), (wv, want)
    print(f"per = {per}, {pred}: s_raw of the kind vs the eps op on the equivalent eps, max |diff| / tolerance {worst:.3f}")


# ---- 4. the loops -------------------------------------------------------------------------------------------------------------------------------------------------

LOOPS = ["ancestral_small", "ancestral_large", "ancestral_learned", "ddim", "ddim_eta", "dpm", "amortized_cfg", "replacement_corrector", "repaint"]


@pytest.mark.parametrize("case", LOOPS)
@pytest.mark.parametrize("pred", ["x0", "v"])
def test_loops_of_a_prediction_chain(nets, case, pred):
    from image_diffusion import sampling
    from image_diffusion.conditioning import ClassifierFreeGuidance, RePaint, Replacement, repaint_walk
    from image_diffusion.likelihoods import InPainting

    base = _chain()
    lik = InPainting(patch_size=6, pad_value=-2)
    xT, cond = _inputs()
    noise = _draws(80)
    net = nets[{"ancestral_learned": (1, 2), "amortized_cfg": (2, 1)}.get(case, (1, 1))]

    def view(chain):
        if case == "ancestral_large":
            chain = chain.with_fixed_variance("large")
        if case == "ancestral_learned":
            chain = chain.with_learned_variance()
        return chain

    r, r_eps = view(base.with_prediction(pred)), view(base)
    assert r.prediction == pred and r.timesteps == base.timesteps and r_eps.prediction == "eps"
    rep = Replacement(0.1, 0.8, True, 1)

    def make(eps_model, chain):
        if case.startswith("ancestral"):
            return sampling.get_prior_sample_fn(eps_model, chain, Replacement(0.1, 1.0, True, 0), lik), (xT.to(DEV),)
        if case in ("ddim", "ddim_eta"):
            return sampling.get_ddim_sample_fn(eps_model, chain, lik, eta=0.5 if case == "ddim_eta" else 0.0), (xT.to(DEV),)
        if case == "dpm":
            return sampling.get_dpm_solver_sample_fn(eps_model, chain, lik, order=2), (xT.to(DEV),)
        if case == "amortized_cfg":
            return sampling.get_conditional_sample_fn(eps_model, chain, ClassifierFreeGuidance(1.0, 1, 0.1, W), lik), (xT.to(DEV), cond.to(DEV))
        cnd = rep if case == "replacement_corrector" else RePaint(0.1, 0.8, True, 0, 2, 2)
        return sampling.get_conditional_sample_fn(eps_model, chain, cnd, lik), (xT.to(DEV), cond.to(DEV))

    def run(eps_model, chain):
        fn, args = make(eps_model, chain)
        with sampling.injected_noise(list(noise)):
            return fn(*args).cpu()

    fast = sampling.make_eps_model(net, r)
    got = run(fast, r)
    gen = run(lambda xi, i: fast(xi, i), r)          # untagged: the host loop over pred_step_
    as_eps = run(sampling.make_eps_model(net, r_eps), r_eps)
    kw = dict(tmin=r.tmin, tmax=r.tmax, delta=0.1)
    if case == "ancestral_learned":
        kw.update(max_log=r.max_log())
    if case in ("ddim", "ddim_eta"):
        kw.update(sampler="ddim", ddim_sigma=r.ddim_sigma(0.5) if case == "ddim_eta" else None)
    if case == "dpm":
        kw.update(sampler="dpmpp", coefs=r.dpm_solver_coefs(2))
    if case == "amortized_cfg":
        kw.update(cond=cond, w=W, n_corrector=1, none_value=-2.0)
    if case in ("replacement_corrector", "repaint"):
        kw.update(replacement=dict(cond=cond, start_fraction=0.8, noise=True, pad=-2.0), n_corrector=1 if case == "replacement_corrector" else 0,
                  walk=repaint_walk(r.Ns, 2, 2) if case == "repaint" else None)
    ref, used, n_eval = PR.sample(_net_out(net, r), r.host_tables(), pred, xT, noise, **kw)
    assert used > 0 or case in ("ddim", "dpm")
    e1 = _report(f"{case}, {pred}: fused vs fp64 restatement", got, ref)
    e2 = _report(f"{case}, {pred}: fused vs host loop", got, gen)
    margin = 5 * (STOL["atol"] + STOL["rtol"] * float(as_eps.abs().max()))
    e3 = _report(f"{case}, {pred}: fused vs the eps-kind result on the same net (margin {margin:.3e})", got, as_eps)
    assert float(got.abs().max()) <= 1.0 and bool(torch.isfinite(got).all()) and (got - xT).abs().max() > 1e-2
    gb = 1e-4 * (1 + 2 * W) if case == "amortized_cfg" else 1e-4
    torch.testing.assert_close(got, gen, rtol=gb, atol=gb)
    torch.testing.assert_close(got.double(), ref, **STOL)
    assert e3 > margin, "the kind is ignored: the result is the eps-kind result"
    assert np.isfinite(e1) and np.isfinite(e2)
    if case == "ancestral_large":      # the fixed large variance moves the result off the fixed small one
        small = run(sampling.make_eps_model(net, base.with_prediction(pred)), base.with_prediction(pred))
        assert _report(f"{case}, {pred}: fixed large vs fixed small", got, small) > margin
    net.engine(DEV).check()


# ---- 5. the bound ---------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", PERS)
def test_vlb_terms_of_a_kind_vs_fp64(per):
    """The kernel evaluates every element in fp64 and rounds each of its three numbers to fp32 once (EPS32); its fp64 evaluation differs from
    numpy's by libm ulps and the order of the sums, orders of magnitude below that: 4 EPS32 relative."""
    from mi355.ops import default_ops as ops

    f32 = np.float32
    for j, (k, sc) in enumerate(vlb_cases()):
        x0, xk, eps, v, z = vlb_operands(per, sc, 700 * j + per)
        kwsc = {name: sc[name] for name in VR.SCALARS}
        as_x0 = (f32(sc["c_recip"]) * xk - f32(sc["c_recipm1"]) * eps).astype(f32)       # the same model, written as each kind writes it
        outs = {"eps": eps, "x0": as_x0, "v": (f32(sc["sa"]) * eps - f32(sc["sb"]) * as_x0).astype(f32)}
        res = {}
        for pred in PREDS:
            for learned in (False, True):
                for clip in (True, False):
                    kw = dict(k_is_zero=k == 0, learned=learned, clip=clip)
                    want = PR.vlb_terms(pred, x0, xk, outs[pred], v, z, sc, sa=sc["sa"], sb=sc["sb"], **kw)
                    out = torch.stack((torch.from_numpy(outs[pred]), torch.from_numpy(v) if learned else torch.full((B, per), float("nan"))), 1)
                    views = [_banded(torch.from_numpy(a).view(B, 1, per), off)[1] for a, off in ((x0, 1), (xk, 3))]
                    zt = torch.from_numpy(z).view(B, 1, per).to(DEV)
                    runs = [ops.vlb_terms(views[0], views[1], _banded(out, 2)[1], z=zt, k_is_zero=k == 0, learned=learned, clip_denoised=clip,
                                          prediction=pred, sa=sc["sa"], sb=sc["sb"], **kwsc).cpu() for _ in range(2)]
                    assert torch.equal(_bits(runs[0]), _bits(runs[1])), "two runs differ"
                    got = runs[0].double().numpy()
                    assert np.isfinite(got).all() and (np.abs(got - want) <= 4 * EPS32 * np.abs(want) + 1e-30).all(), (pred, k, learned, clip, got, want)
                    res[(pred, learned, clip)] = got
        # the mse column is the kind's own: a v-kind run on the same output is not the eps-kind mse
        z_t = torch.from_numpy(z).view(B, 1, per).to(DEV)
        a = [torch.from_numpy(t).view(B, 1, per).to(DEV) for t in (x0, xk)]
        o = torch.from_numpy(eps).view(B, 1, per).to(DEV)
        as_v = ops.vlb_terms(*a, o, z=z_t, k_is_zero=k == 0, learned=False, prediction="v", sa=sc["sa"], sb=sc["sb"], **kwsc).cpu().double().numpy()
        eps_mse = res[("eps", False, True)][:, 2]
        assert (np.abs(as_v[:, 2] - eps_mse) > 100 * 4 * EPS32 * np.abs(eps_mse)).all(), (as_v[:, 2], eps_mse)      # a hundred times the op's tolerance


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("variance", ["fixed_small", "fixed_large", "learned"])
def test_bound_of_a_prediction_chain(nets, pred, variance):
    from image_diffusion import bound, sampling

    base = _chain()
    r = base.with_prediction(pred)
    if variance == "fixed_large":
        r = r.with_fixed_variance("large")
    if variance == "learned":
        r = r.with_learned_variance()
    net = nets[(1, 2) if variance == "learned" else (1, 1)]
    pix = torch.randint(0, 256, (B, 1, S, S), generator=torch.Generator().manual_seed(4243))
    pix.view(-1)[0], pix.view(-1)[1] = 0, 255
    x0 = (pix.float() / 127.5 - 1.0).contiguous()
    noise = randn(8701, 8, B, 1, S, S)
    res = bound.get_vlb_fn(sampling.make_eps_model(net, r), r)(x0.to(DEV), noise=noise.to(DEV))      # variance=None: read from the chain
    got = {f: getattr(res, f).cpu() for f in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")}
    logs = r.vlb_log_variances(variance)
    ref = PR.vlb_loop(_net_out(net, r), r.host_tables(), logs, pred, x0, noise, learned=variance == "learned")
    worst = 0.0
    for f, g in got.items():
        w = torch.from_numpy(np.asarray(ref[f])).double()
        assert bool(torch.isfinite(g).all()), f
        worst = max(worst, float(((g.double() - w).abs() / (STOL["atol"] + STOL["rtol"] * w.abs())).max()))
        torch.testing.assert_close(g.double(), w, **STOL, msg=lambda m, f=f: f"{pred}, {variance}: {f}: {m}")
    print(f"{pred}, {variance}: fused bound vs fp64 restatement, worst |diff| / (atol + rtol |ref|) = {worst:.3e}; total_bpd {got['total_bpd'].tolist()}")
    if pred == "eps":      # the chain's own entry point, bit for bit
        old = bound.get_vlb_fn(sampling.make_eps_model(net, base), base, variance=variance)(x0.to(DEV), noise=noise.to(DEV))
        assert all(torch.equal(_bits(getattr(old, f).cpu()), _bits(g)) for f, g in got.items())
    else:                  # the same net read as an eps net gives another bound and another mse
        other = PR.vlb_loop(_net_out(net, r), r.host_tables(), logs, "eps", x0, noise, learned=variance == "learned")
        margin = STOL["atol"] + STOL["rtol"] * np.abs(other["total_bpd"])
        assert (np.abs(got["total_bpd"].double().numpy() - other["total_bpd"]) > margin).all()
        # (from step 1 on: at step 0 sb is nearly 0 and sa nearly 1, so that v's target sa z - sb x0 is z up to that)
        assert (np.abs(got["mse"].double().numpy() - other["mse"]) > STOL["atol"] + STOL["rtol"] * np.abs(other["mse"]))[:, 1:].all()
    if variance == "fixed_large":
        small = bound.get_vlb_fn(sampling.make_eps_model(net, r), r, variance="fixed_small")(x0.to(DEV), noise=noise.to(DEV))
        gap = (got["total_bpd"].double() - small.total_bpd.cpu().double()).abs()
        assert bool((gap > STOL["atol"] + STOL["rtol"] * small.total_bpd.cpu().double().abs()).all()), "fixed large is fixed small"
    net.engine(DEV).check()


# ---- 6. the public path, the refusals that need a handle ------------------------------------------------------------------------------------------------------------------

def test_public_path_is_one_library_call(nets, monkeypatch):
    from image_diffusion import bound, sampling
    from image_diffusion.conditioning import Amortized, ClassifierFreeGuidance
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib

    lik = InPainting(patch_size=6, pad_value=-2)
    xT, cond = (t.to(DEV) for t in _inputs())
    d = DDPM(25)
    net = nets[(2, 1)]
    eng = net.engine(DEV)
    eng.ddpm_learned(xT.clone(), d.host_tables(), None, mode=_lib.DDPM_PRIOR)
    n_plain = eng.stats(B)["launches"]
    eng.ddpm_learned(xT.clone(), d.host_tables(), None, mode=_lib.DDPM_AMORTIZED, cond=cond, guidance_scale=W)
    n_guided = eng.stats(B)["launches"]
    calls = []
    real = eng.ddpm_pred
    monkeypatch.setattr(eng, "ddpm_pred", lambda *a, **k: calls.append(a[2]) or real(*a, **k))
    for name in ("ddpm_shaped", "ddpm_multistep", "ddpm_learned"):
        monkeypatch.setattr(eng, name, lambda *a, **k: pytest.fail("an entry point without the prediction struct ran"))
    for kind in ("x0", "v"):
        r = d.with_prediction(kind).respace(10)
        em = sampling.make_eps_model(net, r)
        runs = [(sampling.get_prior_sample_fn(em, r, Amortized(1.0, 0, 0.1), lik), (xT,), n_plain, 0),
                (sampling.get_conditional_sample_fn(em, r, ClassifierFreeGuidance(1.0, 0, 0.1, W), lik), (xT, cond), n_guided, 0),
                (sampling.get_conditional_sample_fn(em, r, Amortized(1.0, 0, 0.1), lik), (xT, cond), n_plain, 0),
                (sampling.get_ddim_sample_fn(em, r, lik, guidance_scale=W, eta=0.5), (xT, cond), n_guided, 0),
                (sampling.get_dpm_solver_sample_fn(em, r, lik, guidance_scale=W), (xT, cond), n_guided, 0),
                (sampling.get_ddim_sample_fn(em, r.with_x0_shaping(0.9, guidance_rescale=0.5), lik, guidance_scale=W), (xT, cond), n_guided, 1)]
        for fn, args, n0, stats_launch in runs:
            calls.clear()
            out = fn(*args)
            # no launch is added by the kind: the evaluation, its step launch and, with shaping, the statistics launch
            assert calls == [kind] and eng.stats(B)["launches"] == n0 + stats_launch and n0 > 0, (calls, eng.stats(B)["launches"], n0)
            assert bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0 and (out - xT).abs().max() > 1e-2
    # the bound: one call, through the entry point that takes the kind
    one = nets[(1, 1)]
    e1 = one.engine(DEV)
    seen1 = []
    real1 = e1.ddpm_vlb
    monkeypatch.setattr(e1, "ddpm_vlb", lambda *a, **k: seen1.append(k.get("prediction")) or real1(*a, **k))
    rv = d.with_prediction("v").respace(10)
    res = bound.get_vlb_fn(sampling.make_eps_model(one, rv), rv)(xT.clamp(-1, 1))
    assert seen1 == ["v"] and bool(torch.isfinite(res.total_bpd).all())
    eng.check()
    e1.check()


def test_refusals_that_need_a_handle(nets):
    from mi355 import _lib
    from mi355._lib import MI355BackendError

    r = _chain().with_prediction("v")
    T, ml = r.host_tables(), r.max_log()
    xT, cond = (t.to(DEV) for t in _inputs())
    sched = dict(timesteps=r.timesteps, train_steps=r.base_Ns)
    L = _lib.lib()
    narrow, wide = nets[(2, 1)].engine(DEV), nets[(2, 2)].engine(DEV)
    for kind in ("x0", "v"):
        with pytest.raises(MI355BackendError, match="ddpm_pred_sample: var->learned needs a net whose out_channels == 2 \\* channels"):
            narrow.ddpm_pred(xT.clone(), T, kind, max_log=ml, mode=_lib.DDPM_PRIOR, **sched)
        with pytest.raises(MI355BackendError, match="ddpm_pred_sample: eps model must output the state's channel count"):
            wide.ddpm_pred(xT.clone(), T, kind, mode=_lib.DDPM_PRIOR, **sched)
        with pytest.raises(MI355BackendError, match="ddpm_pred_sample: var->learned together with shaping"):
            wide.ddpm_pred(xT.clone(), T, kind, max_log=ml, shaping=(0.9, None, 0.0), mode=_lib.DDPM_PRIOR, **sched)
        with pytest.raises(MI355BackendError, match="ddpm_pred_sample: replacement needs an unconditional net"):
            narrow.ddpm_pred(xT.clone(), T, kind, mode=_lib.DDPM_REPLACEMENT, cond=cond, **sched)
        with pytest.raises(MI355BackendError, match="ddpm_pred_sample: injected noise exhausted"):
            narrow.ddpm_pred(xT.clone(), T, kind, mode=_lib.DDPM_PRIOR, noise=_draws(2).to(DEV), **sched)
        with pytest.raises(MI355BackendError, match="ddpm_pred_sample: guidance is built for the amortized sampler"):
            narrow.ddpm_pred(xT.clone(), T, kind, mode=_lib.DDPM_PRIOR, cond=cond, guidance_scale=W, **sched)
        with pytest.raises(NotImplementedError, match="tiling.*prediction"):
            narrow.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_PRIOR, prediction=kind, tiling=dict(stride=8), **sched)
        with pytest.raises(NotImplementedError, match="cache_interval.*prediction"):
            narrow.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_PRIOR, prediction=kind, cache_interval=2, **sched)
    with pytest.raises(ValueError, match="prediction must be one of"):
        narrow.ddpm_pred(xT.clone(), T, "xstart", mode=_lib.DDPM_PRIOR, **sched)
    with pytest.raises(MI355BackendError, match="ddpm_pred_sample: workspace too small"):
        ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
        tb, keep = narrow._ddpm_tables(T)
        opt = _lib.DDPMOptionsC(_lib.DDPM_PRIOR, 0, 0.1, 1e-5, 1.0, 1.0, 1, -2.0, -2.0, 1, 0)
        pr = _lib.DDPMPredictionC(2)
        _lib.check(L.mi355_ddpm_pred_sample(narrow.handle, C.c_void_p(xT.data_ptr()), 1, None, None, 0, 0, 0.0, None, C.byref(tb), C.byref(opt), None, None,
                                            None, None, C.byref(pr), None, 0, B, C.c_void_p(ws.data_ptr()), 4096, None), "mi355_ddpm_pred_sample")
    h = narrow.handle
    for guided in (0, 1):
        for multi in (0, 1):
            assert L.mi355_ddpm_pred_workspace_bytes(h, B, guided, multi) == L.mi355_ddpm_shaped_workspace_bytes(h, B, guided, multi)
            assert L.mi355_ddpm_pred_workspace_bytes(wide.handle, B, guided, multi) >= L.mi355_ddpm_lv_workspace_bytes(wide.handle, B, guided, multi)
    # the bound's refusals are mi355_ddpm_vlb's own
    logs = r.vlb_log_variances("fixed_small")
    with pytest.raises(MI355BackendError, match="ddpm_vlb: a fixed variance"):
        wide.ddpm_vlb(xT.clone().clamp(-1, 1), T, logs, learned=False, prediction="v")
    # the step op on device tensors
    from mi355.ops import default_ops as ops
    x, out = torch.zeros(B, 1, 8, device=DEV), torch.zeros(B, 3, 8, device=DEV)
    with pytest.raises(ValueError, match="twice the state's channels"):
        ops.pred_step_("ddpm_lv", "v", x, out, 1.0, 1.0, 0.5, 0.5, min_log=-3.0, max_log=-1.0)
    with pytest.raises(ValueError, match="at least as many channels"):
        ops.pred_step_("ddim", "x0", out, x, 1.0, 1.0, 0.5)
    with pytest.raises(ValueError, match="prediction must be one of"):
        ops.pred_step_("ddim", "xstart", x, x, 1.0, 1.0, 0.5)
    with pytest.raises(MI355BackendError, match="pred_step: the corrector has no guided form"):
        ops.pred_step_("corrector", "v", torch.zeros(2 * B, 1, 8, device=DEV), torch.zeros(2 * B, 2, 8, device=DEV), 1.0, 1.0, 0.5, 0.1, 0.1, w=2.0, sa=0.8, sb=0.6)
    with pytest.raises(MI355BackendError, match="not built for a strided eps"):
        ops.pred_step_("ddim", "v", x, out, 1.0, 1.0, 0.5, sa=0.8, sb=0.6, shape=torch.ones(B, 2, device=DEV))
    narrow.check()
    wide.check()
