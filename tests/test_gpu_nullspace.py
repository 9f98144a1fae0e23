"""GPU: the null-space (DDNM) samplers (mi355_nullspace_step, mi355_block_mean, mi355_ddpm_nullspace_sample; NullSpace, AveragePooling).
  1. the step op against fp64 inside the budget tests/test_nullspace_cpu.py derives: every operator kind x form x prediction kind x {contiguous,
     strided output}, inputs in NaN guard bands at two pointer offsets, two runs bit-identical, a planted NaN giving the reference's NaN pattern;
  2. the bit-exact identities: lam = 0 is mi355_pred_step, the Philox path is the injected mi355_randn draw, mi355_block_mean reproduces the
     kernel's residual, n = 0 does nothing;
  3. the loop with lam = 0 is mi355_ddpm_pred_sample, bit for bit;
  4. the loop against the fp64 restatement driven by the oracle U-Net;
  5. the fused loop against the generic host loop;
  6. the refusals that need a handle and the launch count.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mi355.synth import randn
from oracle import unet_ref
from tests import nullspace_ref as NR
from tests.test_gpu_ddpm_respace import _banded, _bits, _report, _unband
from tests.test_nullspace_cpu import BAND_SHAPES, EPS32, MASK_SHAPES, PREDS, STEPS7, ns_budget, ns_operands, step_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STOL = dict(rtol=2e-3, atol=1e-3)      # SAMPLER_TOL (tests/test_gpu_unet.py): the fused samplers against an fp64 restatement
B, S = 3, 16
KIND_SHAPES = [(0, s) for s in MASK_SHAPES] + [(k, s) for k in (1, 2) for s in BAND_SHAPES]


def _op_struct(op, yshape):
    from mi355.ops import Ops

    return Ops.nullspace_op(op["kind"], yshape, pad_value=-2.0)


def _step_kw(form, c, z):
    return dict(a=c["a"], b=c["b"], lam=c["lam"], sigma=c["sigma"], sa=c["sa"], sb=c["sb"], z=z)


def _launch(ops, op, form, pred, x, out, y, z, c, off, strided):
    """One launch on banded operands at pointer offset `off` floats -> the new state (CPU, flat)."""
    xs = x.shape
    o = torch.from_numpy(out)
    if strided:      # the net's second half: NaN, never read
        o = torch.cat((o, torch.full_like(o, float("nan"))), dim=1)
    bx, vx = _banded(torch.from_numpy(x), off)
    _, vo = _banded(o, off)
    _, vy = _banded(torch.from_numpy(y), off)
    vz = _banded(torch.from_numpy(z), off)[1] if z is not None else None
    assert vx.data_ptr() % 16 == 4 * off
    ops.nullspace_step_(_op_struct(op, y.shape), form, pred, vx, vo, vy, c["cr"], c["crm1"], **_step_kw(form, c, vz))
    torch.cuda.synchronize()
    return _unband(bx, int(np.prod(xs)), off).clone()


# ---- 1. the step op against fp64 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,shape", KIND_SHAPES)
def test_step_vs_fp64(kind, shape):
    from mi355.ops import default_ops as ops

    cases = step_cases()
    worst, seen = {}, set()
    j = 0
    for pred in PREDS:
        for form in (0, 1):
            for strided in (False, True):
                for off in (0, 1):
                    k, f0, f1 = cases[j % len(cases)]
                    j += 1
                    c = f1 if form else f0
                    x, out, y, z, op = ns_operands(kind, shape, pred, c, 300 * j + kind)
                    zz = z if k > 0 else None
                    want, bound = ns_budget(op, pred, form, x, out, y, zz, c)
                    runs = [_launch(ops, op, form, pred, x, out, y, zz, c, off, strided) for _ in range(2)]
                    assert torch.equal(_bits(runs[0]), _bits(runs[1])), "two runs differ"
                    got = runs[0].numpy().reshape(x.shape).astype(np.float64)
                    nan = np.isnan(want)
                    assert np.array_equal(np.isnan(got), nan) and nan.sum() >= 1, (pred, form, strided, off, int(np.isnan(got).sum()), int(nan.sum()))
                    ratio = float((np.abs(got - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max())
                    key = (pred, form)
                    worst[key] = max(worst.get(key, 0.0), ratio)
                    seen.add((pred, form, strided, off))
                    assert not np.array_equal(got[~nan], x.astype(np.float64)[~nan]), "the step did nothing"
    print(f"kind {kind}, {shape}: nullspace_step max err / budget {({k: round(v, 3) for k, v in sorted(worst.items())})}")
    assert len(seen) == 24 and max(worst.values()) <= 1.0, worst


# ---- 2. the bit-exact identities ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,shape", KIND_SHAPES)
def test_lam_zero_is_pred_step(kind, shape):
    from mi355.ops import default_ops as ops

    for j, (k, f0, f1) in enumerate(step_cases()[::2]):
        for pred in PREDS:
            for form, c in ((0, f0), (1, f1)):
                c = dict(c, lam=0.0)
                x, out, y, z, op = ns_operands(kind, shape, pred, c, 50 * j + form, nan=False)
                zz = z if k > 0 else None
                got = _launch(ops, op, form, pred, x, out, y, zz, c, 1, False)
                vx = torch.from_numpy(x).to(DEV)
                zt = torch.from_numpy(zz).to(DEV) if zz is not None else None
                ops.pred_step_("ddim_eta" if form else "ddpm", pred, vx, torch.from_numpy(out).to(DEV), c["cr"], c["crm1"], c["a"], c["b"], sigma=c["sigma"],
                               sa=c["sa"], sb=c["sb"], z=zt)
                assert torch.equal(_bits(got), _bits(vx.cpu().view(-1))), (kind, shape, pred, form, k)


@pytest.mark.parametrize("kind,shape", [(0, MASK_SHAPES[0]), (1, BAND_SHAPES[0]), (2, BAND_SHAPES[1]), (1, BAND_SHAPES[4])])
def test_philox_path_is_the_injected_randn_draw(kind, shape):
    from mi355.ops import default_ops as ops

    k, f0, f1 = step_cases()[2]
    seed, offset = 0x1234567, 4 * 1000
    for form, c in ((0, f0), (1, f1)):
        x, out, y, _, op = ns_operands(kind, shape, "eps", c, 91 + form, nan=False)
        z = ops.randn(x.shape, DEV, seed, offset)
        res = []
        for inject in (True, False):
            vx = torch.from_numpy(x).to(DEV)
            ops.nullspace_step_(_op_struct(op, y.shape), form, "eps", vx, torch.from_numpy(out).to(DEV), torch.from_numpy(y).to(DEV), c["cr"], c["crm1"],
                                a=c["a"], b=c["b"], lam=c["lam"], sigma=c["sigma"], z=z if inject else None, philox=None if inject else (seed, offset))
            res.append(vx.cpu())
        assert torch.equal(_bits(res[0]), _bits(res[1])), (kind, form)
        assert float((res[0] - torch.from_numpy(x)).abs().max()) > 0


@pytest.mark.parametrize("shape", BAND_SHAPES)
def test_block_mean_reproduces_the_residual(shape):
    """lam = 1, coef1 = 1, coef2 = 0, sigma = 0 with an x0-kind output: the step returns x0 - (A(x0) - y) on every element, A summed in the kernel's
    order; mi355_block_mean(x0) - y, spread over the blocks in torch fp32, gives the same bits."""
    from mi355.ops import default_ops as ops

    Bn, Cc, H, W, hl, wl = shape
    sy, sx = H // hl, W // wl
    g = torch.Generator().manual_seed(hl * 100 + wl)
    out = (torch.rand(Bn, Cc, H, W, generator=g) * 3 - 1.5).to(DEV)
    x = torch.randn(Bn, Cc, H, W, generator=g).to(DEV)
    y = (torch.rand(Bn, Cc, hl, wl, generator=g) * 2 - 1).to(DEV)
    x0 = out.clip(-1, 1)
    bx, vin = _banded(x0.cpu(), 1)
    means = [ops.block_mean(vin, (hl, wl)) for _ in range(2)]
    assert torch.equal(_bits(means[0]), _bits(means[1])) and tuple(means[0].shape) == (Bn, Cc, hl, wl)
    ref = torch.nn.functional.avg_pool2d(x0.double(), (sy, sx), (sy, sx))
    assert float((means[0].double() - ref).abs().max()) <= sy * sx * EPS32
    r = means[0] - y
    want = x0 - r.repeat_interleave(sy, dim=2).repeat_interleave(sx, dim=3)
    op = ops.nullspace_op("block_mean", y.shape)
    got = x.clone()
    ops.nullspace_step_(op, 0, "x0", got, out, y, 1.0, 1.0, a=1.0, b=0.0, lam=1.0, sigma=0.0)
    assert bool((got == want).all()), float((got - want).abs().max())      # (== : the step's + 0 * x + 0 * z may turn a -0 into +0)
    assert torch.equal(_bits(got + 0.0), _bits(want * 1.0 + 0.0 * x + 0.0))
    # AveragePooling on device tensors is this op
    from image_diffusion.likelihoods import AveragePooling

    assert torch.equal(_bits(AveragePooling((sy, sx)).sample(x0)), _bits(means[0]))


def test_nothing_to_do():
    from mi355.ops import default_ops as ops

    for kind, yshape in ((0, (0, 2, 8, 12)), (1, (0, 2, 4, 3)), (2, (0, 2, 2, 6))):
        x = torch.empty(0, 2, 8, 12, device=DEV)
        y = torch.empty(yshape, device=DEV)
        assert ops.nullspace_step_(ops.nullspace_op(kind, yshape, pad_value=-2.0), 0, "eps", x, x.clone(), y, 1.0, 1.0, a=1.0) is x
    assert tuple(ops.block_mean(torch.empty(0, 2, 8, 12, device=DEV), (4, 3)).shape) == (0, 2, 4, 3)
    torch.cuda.synchronize()


# ---- nets, chains, inputs ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets():
    from tests.test_gpu_unet import _tiny

    return {(1, 1): _tiny(1, 1, 1001, "fp32"), (3, 6): _tiny(3, 6, 1021, "fp32")}      # (in, out channels) -> (cfg, net, sd)


def _chain():
    from image_diffusion.sde_diffusion import DDPM

    return DDPM(100).respace(STEPS7)


def _inputs(Cc=1):
    xT = randn(9101, B, Cc, S, S)
    truth = (randn(9102, B, Cc, S, S) * 0.5).clamp(-1, 1)
    return xT, truth


def _draws(n, Cc=1):
    return [randn(9200 + j, B, Cc, S, S) for j in range(n)]


def _likelihood(kind):
    from image_diffusion.likelihoods import AveragePooling, InPainting, LowResolution

    return {0: InPainting(patch_size=6, pad_value=-2), 1: AveragePooling(4), 2: LowResolution(8, 4)}[kind]


def _measure(kind, truth):
    """-> (the measurement as the likelihoods make it, on the CPU; the restatement's operator)."""
    if kind == 0:
        y = truth.clone()
        y[:, :, 4:10, 5:11] = -2.0
        return y, dict(kind=0, known=(y != -2.0).numpy())
    y = _likelihood(kind).sample(truth.to(DEV)).cpu()
    return y, (dict(kind=1, hl=4, wl=4) if kind == 1 else dict(kind=2, hl=8, wl=4))


def _libm_expf(v):
    libm = C.CDLL("libm.so.6")
    libm.expf.restype, libm.expf.argtypes = C.c_float, [C.c_float]
    return libm.expf(C.c_float(v))


# ---- 3. the loop anchor -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", ["7of100", "full25"])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("noise", ["injected", "philox"])
def test_lam_zero_loop_is_ddpm_pred_sample(nets, sched, form, noise):
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib
    from mi355.ops import default_ops as ops

    r = _chain() if sched == "7of100" else DDPM(25)
    K = r.Ns
    T = r.host_tables()
    eng = nets[(1, 1)][1].engine(DEV)
    xT, truth = _inputs()
    kw = dict(mode=_lib.DDIM if form else _lib.DDPM_PRIOR, seed=77)
    if noise == "injected":
        kw["noise"] = torch.stack(_draws(K)).to(DEV)
    if sched == "7of100":
        kw.update(timesteps=r.timesteps, train_steps=r.base_Ns)
    if form and sched == "7of100":
        kw["ddim_sigma"] = r.ddim_sigma(0.85)
    # the posterior's sigma as the library's own loop forms it: expf(0.5f * logvar) on the host
    sig = [_libm_expf(float(np.float32(0.5) * T["posterior_log_variance_clipped"][i].numpy())) for i in range(K)] if form == 0 else None
    want = eng.ddpm_pred(xT.to(DEV).clone(), T, "eps", **kw).cpu()
    for kind in (0, 1, 2):
        y, _ = _measure(kind, truth)
        got = eng.ddpm_nullspace(xT.to(DEV).clone(), T, y.to(DEV), ops.nullspace_op(kind, y.shape, pad_value=-2.0), [0.0] * K, sig, **kw).cpu()
        assert torch.equal(_bits(got), _bits(want)), (kind, float((got - want).abs().max()))
    assert float((want - xT).abs().max()) > 1e-2
    eng.check()


# ---- 4., 5. the loop against the fp64 restatement on the oracle U-Net, and against the generic host loop ---------------------------------------------------

LOOPS = ["mask_f0", "mask_f1", "pool_f0", "pool_f1", "bilinear_f0", "bilinear_f1", "mask_plus", "pool_plus", "pool_walk", "mask_walk_f1", "bilinear_v",
         "pool_wide_f1", "mask_labels"]


@pytest.mark.parametrize("case", LOOPS)
def test_loop_vs_restatement_and_host_loop(nets, case):
    from image_diffusion import sampling
    from image_diffusion.conditioning import NullSpace, repaint_walk

    kind = {"mask": 0, "pool": 1, "bilinear": 2}[case.split("_")[0]]
    form = 1 if case.endswith("f1") else 0
    sigma_y = 0.3 if case.endswith("plus") else 0.0
    jump = (2, 2) if "walk" in case else (1, 1)
    wide, labelled = "wide" in case, "labels" in case
    pred = "v" if case.endswith("_v") else "eps"
    Cc = 3 if wide else 1
    r = _chain()
    chain = r.with_prediction(pred) if pred != "eps" else r
    if wide:
        chain = chain.with_learned_variance()
    cnd = NullSpace(sigma_y, 0.5 if form else None, *jump)
    lik = _likelihood(kind)
    xT, truth = _inputs(Cc)
    y, op = _measure(kind, truth)
    draws = _draws(3 * r.Ns, Cc)
    labels = None
    if labelled:
        from tests.test_classcond_cpu import ClassCondConfig, classcond_forward
        from tests.test_gpu_classcond import _model

        cfg = ClassCondConfig(16, 1, 32, 1, 1, (2,), channel_mult=(1, 2), num_heads=2, num_classes=5)
        net, sd = _model(cfg, 1031, "fp32")
        labels = torch.tensor([4, 0, 2])
        oracle = lambda x, k: classcond_forward(sd, cfg, torch.from_numpy(x), torch.full((B,), chain.time(k), dtype=torch.float32), labels).numpy()   # noqa: E731
    else:
        cfg, net, sd = nets[(3, 6) if wide else (1, 1)]
        oracle = lambda x, k: unet_ref.unet_forward(sd, cfg, torch.from_numpy(x), torch.full((B,), chain.time(k), dtype=torch.float32)).numpy()   # noqa: E731
    fast = sampling.make_eps_model(net, chain)
    extra = dict(y=labels.to(DEV)) if labelled else {}
    with sampling.injected_noise(draws):
        got = sampling.get_conditional_sample_fn(fast, chain, cnd, lik)(xT.to(DEV), y.to(DEV), **extra).cpu()
    lam, sig = chain.nullspace_coefs(sigma_y)
    dsig = chain.ddim_sigma(0.5).numpy() if form else None
    walk = repaint_walk(r.Ns, *jump) if jump != (1, 1) else None
    T = {k: v.numpy() for k, v in chain.host_tables().items()}
    ref, used, n_eval = NR.sample(oracle, T, op, pred, form, xT.numpy(), y.numpy(), [d.numpy() for d in draws], lam.numpy(), sig.numpy(), dsig, walk,
                                  channels=Cc)
    ref = torch.from_numpy(ref)
    e1 = _report(f"{case}: fused vs fp64 restatement on the oracle U-Net ({n_eval} evaluations, {used} draws)", got, ref)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 1.0 and float((got - xT).abs().max()) > 1e-2
    torch.testing.assert_close(got.double(), ref, **STOL)
    # exactly the draws the restatement used
    if used:
        from mi355._lib import MI355BackendError

        with sampling.injected_noise(draws[:used - 1]), pytest.raises(MI355BackendError, match="injected noise exhausted"):
            sampling.get_conditional_sample_fn(fast, chain, cnd, lik)(xT.to(DEV), y.to(DEV), **extra)
    if not labelled:      # the generic host loop over nullspace_step_ (an untagged callable)
        with sampling.injected_noise(draws):
            gen = sampling.get_conditional_sample_fn(lambda xi, i: fast(xi, i), chain, cnd, lik)(xT.to(DEV), y.to(DEV)).cpu()
        e2 = _report(f"{case}: fused vs generic host loop", got, gen)
        torch.testing.assert_close(got, gen, rtol=1e-4, atol=1e-4)
        assert np.isfinite(e2)
    if kind == 0 and sigma_y == 0.0:      # plain DDNM: the known pixels of the result are the measurement, to the last step's budget
        known = torch.from_numpy(op["known"])
        c1 = float(T["posterior_mean_coef1"][0]) if form == 0 else 1.0
        slack = ((got - y).abs() - (4 * EPS32 * (1 + y.abs()) + abs(c1 - 1) * y.abs()))[known]
        print(f"{case}: known pixels vs the measurement, max|diff| {float((got - y).abs()[known].max()):.3e}")
        assert float(slack.max()) <= 0
    if kind == 1 and sigma_y == 0.0 and not wide:      # and the block means of the result are the measurement where the final clip does not act
        from mi355.ops import default_ops as ops

        inside = (got.abs() < 1).reshape(B, Cc, 4, 4, 4, 4).all(dim=5).all(dim=3)
        d = (ops.block_mean(got.to(DEV), (4, 4)).cpu() - y).abs()[inside]
        worst = float(d.max()) if d.numel() else 0.0      # (an untrained net saturates most blocks: there may be none)
        print(f"{case}: block means of the result vs the measurement on {int(inside.sum())} unclipped blocks, max|diff| {worst:.3e}")
        assert worst <= 64 * EPS32
    assert np.isfinite(e1)
    net.engine(DEV).check()


# ---- 6. refusals and the launch count ------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(nets):
    from mi355 import _lib
    from mi355.ops import Ops

    L = _lib.lib()
    r = _chain()
    K = r.Ns
    T = r.host_tables()
    xT, truth = _inputs()
    x = xT.to(DEV).clone()
    y1 = _measure(1, truth)[0].to(DEV)
    FP = C.POINTER(C.c_float)
    fl = lambda v: (C.c_float * K)(*v)   # noqa: E731
    lam_ok, sig_ok = fl([1.0] * K), fl([0.1] * K)
    e1 = nets[(1, 1)][1].engine(DEV)
    e6 = nets[(3, 6)][1].engine(DEV)
    from tests.test_gpu_unet import _tiny

    e2 = _tiny(2, 1, 1002, "fp32")[1].engine(DEV)      # a 2C-input (amortized) net
    good = Ops.nullspace_op(1, y1.shape)

    def call(eng=e1, mode=_lib.DDPM_PRIOR, op=good, lam=lam_ok, sigma=sig_ok, n_corrector=0, channels=1, y=y1, ns=True, short=False, labels=None, xx=None):
        tb, keep = eng._ddpm_tables(T)
        opt = _lib.DDPMOptionsC(mode, n_corrector, 0.1, 1e-5, 1.0, 1.0, 1, -2.0, -2.0, 0, 0)
        nsc = _lib.NullspaceScheduleC(C.cast(lam, FP) if lam is not None else None, C.cast(sigma, FP) if sigma is not None else None)
        ws, wsb = eng._workspace_sized("mi355_ddpm_nullspace_workspace_bytes", B)      # (the engine's buffer may be larger than this call needs)
        need = L.mi355_ddpm_nullspace_workspace_bytes(eng.handle, B)
        assert 0 < need <= wsb
        return L.mi355_ddpm_nullspace_sample(eng.handle, C.c_void_p((xx if xx is not None else x).data_ptr()), channels,
                                             C.c_void_p(y.data_ptr()) if y is not None else None, C.byref(op) if op is not None else None, labels,
                                             C.byref(tb), C.byref(opt), None, C.byref(nsc) if ns else None, None, None, 0, B, ws, need - 1 if short else wsb,
                                             None)

    O = _lib.NullspaceOpC
    bad = [(dict(y=None), -1, "y is null"), (dict(op=None), -1, "op is null"), (dict(ns=False), -1, "ns is null"), (dict(sigma=None), -1, "ns->sigma is null"),
           (dict(mode=_lib.DDIM), -1, "ns->sigma given in form 1"), (dict(lam=fl([1.0] * 3 + [-0.5] + [1.0] * 3)), -1, "ns->lam"),
           (dict(lam=fl([float("nan")] + [1.0] * 6)), -1, "ns->lam"), (dict(lam=fl([1.0] * 6 + [1.5])), -1, "ns->lam must be <= 1"),
           (dict(sigma=fl([0.1] * 6 + [float("inf")])), -1, "ns->sigma"), (dict(sigma=fl([-0.1] + [0.1] * 6)), -1, "ns->sigma"),
           (dict(n_corrector=1), -1, "n_corrector"), (dict(mode=_lib.DDPM_AMORTIZED), -1, "opt->mode"), (dict(mode=_lib.DDPM_REPLACEMENT), -1, "opt->mode"),
           (dict(eng=e2), -2, "unconditional net"), (dict(eng=e6, channels=3), -2, "2C-output"), (dict(op=O(3, 0.0, 4, 4)), -1, "op->kind"),
           (dict(op=O(1, 0.0, 0, 4)), -1, "op->h_low"), (dict(op=O(2, 0.0, 4, -2)), -1, "op->h_low"), (dict(op=O(1, 0.0, 5, 4)), -4, "integer factors"),
           (dict(op=O(2, 0.0, 4, 3)), -4, "integer factors"), (dict(short=True), -2, "workspace too small"),
           (dict(labels=C.c_void_p(x.data_ptr())), -1, "labels")]
    for kw, code, word in bad:
        rc = call(**kw)
        assert rc == code and word.encode() in L.mi355_last_error(), (kw, rc, L.mi355_last_error())
    torch.cuda.synchronize()
    assert torch.equal(_bits(x.cpu()), _bits(xT))      # nothing was launched: the state is untouched, byte for byte
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(x.cpu(), xT)
    x6 = randn(9301, B, 3, S, S).to(DEV)
    y6 = _measure(1, (randn(9302, B, 3, S, S) * 0.5).clamp(-1, 1))[0].to(DEV)
    assert call(eng=e6, channels=3, mode=_lib.DDIM, sigma=None, y=y6, op=Ops.nullspace_op(1, y6.shape), xx=x6) == 0      # form 1 reads a 2C-output net
    torch.cuda.synchronize()
    # the step op's refusals on device operands
    from mi355._lib import MI355BackendError
    from mi355.ops import default_ops as ops

    xs = xT.to(DEV).clone()
    for kw, word in ((dict(lam=1.5), "lam"), (dict(sigma=-1.0), "sigma"), (dict(philox=(1, 6)), "multiple of 4")):
        with pytest.raises(MI355BackendError, match=word):
            ops.nullspace_step_(good, 0, "eps", xs, xs.clone(), y1, 1.0, 1.0, **dict(dict(a=1.0, b=0.0), **kw))
    with pytest.raises(MI355BackendError, match="1..32"):
        big = torch.zeros(1, 1, 33, 66, device=DEV)
        ops.nullspace_step_(Ops.nullspace_op(2, (1, 1, 1, 2)), 0, "eps", big, big.clone(), torch.zeros(1, 1, 1, 2, device=DEV), 1.0, 1.0, a=1.0)
    with pytest.raises(ValueError, match="measurement"):
        ops.nullspace_step_(good, 0, "eps", xs, xs.clone(), y1[:, :, :2], 1.0, 1.0, a=1.0)
    torch.cuda.synchronize()
    assert torch.equal(_bits(xs.cpu()), _bits(xT))
    for e in (e1, e2, e6):
        e.check()


def test_launch_count_is_the_evaluations_plus_one(nets):
    from mi355 import _lib
    from mi355.ops import default_ops as ops

    r = _chain()
    T = r.host_tables()
    eng = nets[(1, 1)][1].engine(DEV)
    xT, truth = _inputs()
    t = torch.full((B,), r.time(0), device=DEV)
    eng.forward(xT.to(DEV), t)
    n_fwd = eng.stats(B)["launches"]
    eng.ddpm_sample(xT.to(DEV).clone(), T, mode=_lib.DDPM_PRIOR, seed=3, timesteps=r.timesteps, train_steps=r.base_Ns)
    n_eval = eng.stats(B)["launches"]      # the scheduled loop reports its last evaluation
    lam, sig = r.nullspace_coefs(0.0)
    for kind in (0, 1, 2):
        y = _measure(kind, truth)[0].to(DEV)
        for form in (0, 1):
            eng.ddpm_nullspace(xT.to(DEV).clone(), T, y, ops.nullspace_op(kind, y.shape, pad_value=-2.0), lam, sig if form == 0 else None,
                               mode=_lib.DDIM if form else _lib.DDPM_PRIOR, seed=3, timesteps=r.timesteps, train_steps=r.base_Ns)
            n = eng.stats(B)["launches"]
            print(f"kind {kind}, form {form}: {n} launches in the last step (one forward: {n_fwd}; the scheduled loop's last evaluation: {n_eval})")
            assert n == n_eval + 1 and n_eval > 0
    eng.check()
