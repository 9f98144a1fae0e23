"""GPU: feature reuse across sampler steps (DeepCache) on the HIP path - a shallow evaluation against the restatement
(tests/feature_cache_ref.py), its identity with the full evaluation, launch accounting, the large-tile kernels at a bench-sized batch, the cached
Euler and DDPM samplers against the fp64 restatement and against a host-driven loop, the drift kernel and the samplers' drift_out, and the
refusals through the C ABI.

Tolerances are the project's own for the same arithmetic: the forward's fp32 bound rtol 2e-4 / atol 5e-5 and bf16 bound (tests/test_gpu_unet.py),
the batch-against-single-image bounds 2e-5 / 3e-2, the Euler-trajectory bound 5e-4 / 5e-5, SAMPLER_TOL for the DDPM loops.  A GPU path that ignored
the cache, or recomputed everything, would be off by 0.9 to 1.9 at an output scale of 1.5 (tests/test_feature_cache_cpu.py).
"""
import ctypes as C
import functools

import pytest
import torch

from mi355.synth import randn
from oracle import cfm_ref, unet_ref
from oracle.unet_ref import UNetConfig
from tests import ddpm_respace_ref as DR
from tests import feature_cache_ref as R
from tests.test_feature_cache_cpu import CIFAR, TINY, tiny_inputs, tiny_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAMPLER_TOL = dict(rtol=2e-3, atol=1e-3)   # tests/test_gpu_unet.py
B2 = 2


@functools.lru_cache(maxsize=None)
def _net(idx, precision):
    from tests.test_gpu_unet import build

    return build(TINY[idx], 1003, precision)[0]


@functools.lru_cache(maxsize=None)
def _ref_shallow(idx, k):
    """(full(x0, t0), the restatement's shallow(x1, t1) on F(x0, t0)), computed once per (net, branch)."""
    x0, t0, x1, t1 = tiny_inputs()
    y0, feat = R.full_with_feature(tiny_sd(idx), TINY[idx], x0, t0, k)
    return y0, R.shallow(tiny_sd(idx), TINY[idx], x1, t1, k, feat)


def _report(tag, got, ref):
    err = (got.double() - ref.double()).abs()
    scale = float(ref.abs().max())
    rms = float(err.pow(2).mean().sqrt()) / max(float(ref.double().pow(2).mean().sqrt()), 1e-12)
    print(f"{tag}: max|err| {float(err.max()):.3e} (scale {scale:.3f}), rel rms {rms:.3e}")
    return float(err.max()), scale, rms


# ---- 1. op level, against the oracle -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("idx", [0, 1])
def test_shallow_forward_vs_restatement(idx, precision, k):
    eng = _net(idx, precision).engine(DEV)
    x0, t0, x1, t1 = (v.to(DEV) for v in tiny_inputs())
    y0, ref = _ref_shallow(idx, k)
    full = eng.forward(x0, t0).cpu()
    got = eng.forward_cached(x1, t1, branch=k).cpu()
    eng.check()
    err, scale, rms = _report(f"net {idx} {precision} branch {k}: shallow vs restatement", got, ref)
    print(f"   (ignoring the cache would be off by {float((ref - y0).abs().max()):.2f})")
    if precision == "fp32":
        torch.testing.assert_close(full, y0, rtol=2e-4, atol=5e-5)
        torch.testing.assert_close(got, ref, rtol=2e-4, atol=5e-5)
    else:
        assert err < 0.04 * scale and rms < 0.02


@pytest.mark.parametrize("precision", ["bf16x2", "fp16"])
def test_shallow_forward_other_precisions(precision):
    """The two remaining precisions on the plain tiny net at the branch that crosses the 8x8 level, held to bf16's bound."""
    eng = _net(0, precision).engine(DEV)
    x0, t0, x1, t1 = (v.to(DEV) for v in tiny_inputs())
    eng.forward(x0, t0)
    got = eng.forward_cached(x1, t1, branch=3).cpu()
    eng.check()
    err, scale, rms = _report(f"{precision} branch 3: shallow vs restatement", got, _ref_shallow(0, 3)[1])
    assert err < 0.04 * scale and rms < 0.02


# ---- 2. identity ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("idx", [0, 1])
def test_shallow_at_the_same_input_is_the_full_forward(idx, precision):
    eng = _net(idx, precision).engine(DEV)
    x0, t0, _, _ = (v.to(DEV) for v in tiny_inputs())
    a = eng.forward(x0, t0).clone()
    b = eng.forward(x0, t0).clone()
    deterministic = torch.equal(a, b)
    print(f"net {idx} {precision}: two full forwards of one input are {'bit-identical' if deterministic else 'NOT bit-identical'}")
    for k in (1, 2, 3):
        eng.forward(x0, t0)
        s = eng.forward_cached(x0, t0, branch=k)
        print(f"   branch {k}: max|shallow - full| {float((s - a).abs().max()):.3e}")
        if deterministic:
            assert torch.equal(s, a), k   # same kernels, same inputs
        else:
            torch.testing.assert_close(s, a, rtol=1e-5, atol=3e-6)   # the bound of test_batch_independence_and_large_batch
    eng.check()


# ---- 3. launch accounting ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx", [0, 1])
def test_launch_accounting_and_skipped_tensors(idx):
    from mi355._lib import MI355BackendError

    eng = _net(idx, "fp32").engine(DEV)
    x0, t0, x1, t1 = (v.to(DEV) for v in tiny_inputs())
    prof = eng.profile(x0, t0)                     # record 0: the prelude; record 1 + i: plan op i (tile (-1, -1): nothing launched)
    ops = eng.plan_ops()
    assert len(prof) == len(ops) + 1
    for br in eng.cache_branches():
        k, (lo, hi), tid = br["branch"], br["skip_ops"], br["tensor"]
        assert ops[hi - 1]["dst"] == tid and tuple(br["shape"][:2]) == (ops[hi - 1]["dst_c"], ops[hi - 1]["dst_h"])
        eng.forward(x0, t0)
        n_full = eng.stats(B2)["launches"]
        # the tensors the skipped range's convs and attention ops wrote, as the full evaluation left them
        kept = {}
        for op in ops[lo:hi]:
            if op["kind"] in (1, 2, 5) and op["dst"] >= 0:
                try:
                    kept[op["dst"]] = eng.read_tensor(op["dst"], B2, (op["dst_c"], op["dst_h"], op["dst_h"])).clone()
                except MI355BackendError:
                    pass   # not materialised by the full forward either (fused into its consumer)
        assert tid in kept and len(kept) >= 3
        first = eng.read_tensor(ops[0]["dst"], B2, (ops[0]["dst_c"], ops[0]["dst_h"], ops[0]["dst_h"])).clone()
        eng.forward_cached(x1, t1, branch=k)
        n_shallow = eng.stats(B2)["launches"]
        skipped = sum(1 for r in prof[1 + lo:1 + hi] if tuple(r["tile"]) != (-1, -1))
        print(f"net {idx} branch {k}: launches {n_full} full, {n_shallow} shallow; plan ops [{lo}, {hi}) hold {skipped} launches")
        assert n_shallow < n_full and n_shallow == n_full - skipped
        assert eng.plan_ops() == ops
        for t, v in kept.items():
            op = next(o for o in ops if o["dst"] == t)
            assert torch.equal(eng.read_tensor(t, B2, (op["dst_c"], op["dst_h"], op["dst_h"])), v), t
        assert not torch.equal(eng.read_tensor(ops[0]["dst"], B2, (ops[0]["dst_c"], ops[0]["dst_h"], ops[0]["dst_h"])), first)
    eng.check()


def test_engine_tracks_whether_its_workspace_holds_a_full_evaluation():
    from mi355._lib import MI355BackendError

    eng = _net(0, "fp32").engine(DEV)
    x0, t0, x1, t1 = (v.to(DEV) for v in tiny_inputs())
    eng.forward(x0, t0)
    eng.forward_cached(x1, t1, branch=1)
    eng.forward_cached(x1, t1, branch=2)           # shallow after shallow: the full evaluation is still there
    eng.cfm_euler(x0.clone(), [0.0, 0.5, 1.0])     # a sampler ran the net: the mark is gone
    with pytest.raises(MI355BackendError, match="full evaluation"):
        eng.forward_cached(x1, t1, branch=1)
    eng.forward_cached(x0, t0, branch=0)
    eng.forward_cached(x1, t1, branch=1)
    with pytest.raises(MI355BackendError, match="full evaluation"):   # another batch: another layout of the workspace
        eng.forward_cached(x1[:1].contiguous(), t1[:1].contiguous(), branch=1)
    eng.profile(x0, t0)
    with pytest.raises(MI355BackendError, match="full evaluation"):
        eng.forward_cached(x1, t1, branch=1)
    eng.check()


# ---- 4. the large-tile kernels -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,tol", [("fp32", 2e-5), ("bf16", 3e-2)])
def test_headline_unet_shallow_bench_batch_matches_single_images(precision, tol):
    """The CIFAR net at B = 96, branch 3 (finalize-from-partial-sums, carried skip convs, ping-pong / warp-specialised routes on the retained
    side): full then shallow at B = 96 against the same images run alone, full then shallow.  Pattern and bounds of
    test_headline_unet_bench_batch_matches_single_images."""
    from tests.test_gpu_unet import build

    net, _ = build(CIFAR, 77, precision)
    eng = net.engine(DEV)
    Bn, k = 96, 3
    x0, x1 = randn(5, Bn, 3, 32, 32).to(DEV), randn(6, Bn, 3, 32, 32).to(DEV)
    t0, t1 = torch.linspace(0, 1, Bn).to(DEV), torch.linspace(1, 0, Bn).to(DEV)
    f = eng.forward(x0, t0).clone()
    y = eng.forward_cached(x1, t1, branch=k).clone()
    assert torch.isfinite(y).all() and float((y - f).abs().max()) > 0.1
    for i in (0, 41, 95):
        eng.forward(x0[i:i + 1].contiguous(), t0[i:i + 1].contiguous())
        yi = eng.forward_cached(x1[i:i + 1].contiguous(), t1[i:i + 1].contiguous(), branch=k)
        print(f"{precision} image {i}: max|batch - alone| {float((y[i:i + 1] - yi).abs().max()):.3e}")
        torch.testing.assert_close(y[i:i + 1], yi, rtol=tol, atol=tol)
    eng.check()


@pytest.mark.parametrize("k", [5, 8])
def test_cifar_net_deep_branches_vs_restatement(k):
    """What the tiny nets' channel counts do not reach: on the CIFAR net the concat norm of output_blocks[n-k] has whole groups in each source, so
    at the 8x8 level (k = 8) both producers apply their halves in their epilogues and the shallow evaluation reads the half the skipped producer
    left; at the 16x16 level (k = 5) the norm is finalized from partial sums, the cached tensor's from the full evaluation.  fp32, B = 2,
    against the restatement at the forward's bound, and the identity."""
    from tests.test_gpu_unet import build

    net, sd = build(CIFAR, 77, "fp32")
    eng = net.engine(DEV)
    x0, x1 = randn(11, B2, 3, 32, 32), randn(12, B2, 3, 32, 32)
    t0, t1 = torch.tensor([0.2, 0.7]), torch.tensor([0.5, 0.9])
    y0, feat = R.full_with_feature(sd, CIFAR, x0, t0, k)
    ref = R.shallow(sd, CIFAR, x1, t1, k, feat)
    full = eng.forward(x0.to(DEV), t0.to(DEV)).clone()
    got = eng.forward_cached(x1.to(DEV), t1.to(DEV), branch=k).cpu()
    _report(f"CIFAR net branch {k}: shallow vs restatement", got, ref)
    print(f"   (ignoring the cache would be off by {float((ref - y0).abs().max()):.2f})")
    assert float((ref - y0).abs().max()) > 0.1
    torch.testing.assert_close(full.cpu(), y0, rtol=2e-4, atol=5e-5)
    torch.testing.assert_close(got, ref, rtol=2e-4, atol=5e-5)
    deterministic = torch.equal(eng.forward(x0.to(DEV), t0.to(DEV)), full)
    same = eng.forward_cached(x0.to(DEV), t0.to(DEV), branch=k)
    print(f"   two full forwards are {'bit-identical' if deterministic else 'NOT bit-identical'}; max|shallow - full| at the same input {float((same - full).abs().max()):.3e}")
    if deterministic:
        assert torch.equal(same, full)
    else:
        torch.testing.assert_close(same, full, rtol=1e-5, atol=3e-6)
    eng.check()


# ---- 5. the Euler sampler ----------------------------------------------------------------------------------------------------------------------

N_STEPS = 6
EULER_SCHEDULES = {"interval3": dict(cache_interval=3), "list": dict(cache_schedule=[1, 0, 1, 1, 0, 0])}


def _full_list(kw):
    return R.interval_schedule(N_STEPS, kw["cache_interval"]) if "cache_interval" in kw else [bool(f) for f in kw["cache_schedule"]]


def _host_loop(eng, x0, ts, k, full, **kw):
    """forward / forward_cached plus the Euler step kernel, driven from the host."""
    from mi355.ops import default_ops

    x = x0.clone()
    out = [x.clone()]
    for j in range(len(ts) - 1):
        c = kw.get("cond")
        v = eng.forward_cached(x, ts[j], cond=c, y=kw.get("y"), branch=0 if full[j] else k)
        default_ops.euler_step_(x, v, ts[j + 1] - ts[j])
        out.append(x.clone())
    return torch.stack(out)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("idx", [0, 1])
def test_cached_euler(idx, k):
    eng = _net(idx, "fp32").engine(DEV)
    x0 = randn(1, B2, 3, 16, 16)
    tsp = torch.linspace(0, 1, N_STEPS + 1)
    ts = tsp.tolist()
    plain = eng.cfm_euler(x0.to(DEV), ts, keep_traj=True, want_u8=True)
    allfull = eng.cfm_euler(x0.to(DEV), ts, keep_traj=True, want_u8=True, cache_interval=1, cache_branch=k)
    for a, b in zip(plain, allfull):
        assert torch.equal(a, b)   # caching nothing is the uncached sampler, bit for bit
    for name, kw in EULER_SCHEDULES.items():
        full = _full_list(kw)
        ref, _ = R.cached_euler(tiny_sd(idx), TINY[idx], x0, tsp, k, full)
        x, traj, u8 = eng.cfm_euler(x0.to(DEV), ts, keep_traj=True, want_u8=True, cache_branch=k, **kw)
        host = _host_loop(eng, x0.to(DEV), ts, k, full)
        _report(f"net {idx} branch {k} {name}: cached Euler vs fp64 restatement", traj.cpu(), ref)
        _report(f"net {idx} branch {k} {name}: cached Euler vs host loop", traj, host)
        print(f"   (the schedule moves the end state by {float((traj[-1] - plain[1][-1]).abs().max()):.3e})")
        assert float((traj[-1] - plain[1][-1]).abs().max()) > 1e-3
        torch.testing.assert_close(traj.cpu().double(), ref, rtol=5e-4, atol=5e-5)
        torch.testing.assert_close(traj, host, rtol=1e-5, atol=1e-6)
        assert torch.equal(x, traj[-1])
        assert (u8.cpu().int() - cfm_ref.to_uint8(ref[-1].float()).int()).abs().max() <= 1
    eng.check()


def test_cached_euler_with_labels(golden):
    from tests.test_classcond_cpu import load_case
    from tests.test_gpu_classcond import _model

    g, cfg = load_case(golden, "tiny")
    net, sd = _model(cfg, int(g["seed"]), "fp32")
    eng = net.engine(DEV)
    x0 = randn(3, B2, cfg.in_channels, cfg.image_size, cfg.image_size)
    y = torch.tensor([1, cfg.num_classes - 1])
    tsp = torch.linspace(0, 1, N_STEPS + 1)
    ts, k, kw = tsp.tolist(), 3, EULER_SCHEDULES["interval3"]
    full = _full_list(kw)
    ref, _ = R.cached_euler(sd, cfg, x0, tsp, k, full, y=y)
    plain = eng.cfm_euler(x0.to(DEV), ts, keep_traj=True, y=y.to(DEV))
    allfull = eng.cfm_euler(x0.to(DEV), ts, keep_traj=True, y=y.to(DEV), cache_interval=1, cache_branch=k)
    assert torch.equal(plain[1], allfull[1])
    _, traj, u8 = eng.cfm_euler(x0.to(DEV), ts, keep_traj=True, want_u8=True, y=y.to(DEV), cache_branch=k, **kw)
    host = _host_loop(eng, x0.to(DEV), ts, k, full, y=y.to(DEV))
    _report("labels: cached Euler vs fp64 restatement", traj.cpu(), ref)
    torch.testing.assert_close(traj.cpu().double(), ref, rtol=5e-4, atol=5e-5)
    torch.testing.assert_close(traj, host, rtol=1e-5, atol=1e-6)
    assert (u8.cpu().int() - cfm_ref.to_uint8(ref[-1].float()).int()).abs().max() <= 1
    eng.check()


def test_cached_euler_with_condition():
    from tests.test_gpu_unet import _tiny

    cfg, net, sd = _tiny(6, 3, 1006, "fp32")
    eng = net.engine(DEV)
    x0, cond = randn(4, B2, 3, 16, 16), randn(5, B2, 3, 16, 16)
    tsp = torch.linspace(0, 1, N_STEPS + 1)
    ts, k, kw = tsp.tolist(), 1, EULER_SCHEDULES["list"]
    full = _full_list(kw)
    ref, _ = R.cached_euler(sd, cfg, x0, tsp, k, full, cond=cond)
    plain = eng.cfm_euler(x0.to(DEV), ts, cond=cond.to(DEV), keep_traj=True)
    allfull = eng.cfm_euler(x0.to(DEV), ts, cond=cond.to(DEV), keep_traj=True, cache_interval=1)
    assert torch.equal(plain[1], allfull[1])
    _, traj, u8 = eng.cfm_euler(x0.to(DEV), ts, cond=cond.to(DEV), keep_traj=True, want_u8=True, cache_branch=k, **kw)
    host = _host_loop(eng, x0.to(DEV), ts, k, full, cond=cond.to(DEV))
    _report("condition: cached Euler vs fp64 restatement", traj.cpu(), ref)
    torch.testing.assert_close(traj.cpu().double(), ref, rtol=5e-4, atol=5e-5)
    torch.testing.assert_close(traj, host, rtol=1e-5, atol=1e-6)
    assert (u8.cpu().int() - cfm_ref.to_uint8(ref[-1].float()).int()).abs().max() <= 1
    # slices beyond max_batch() are calls of their own
    eng.max_batch_override = 1
    try:
        _, tr2, _ = eng.cfm_euler(x0.to(DEV), ts, cond=cond.to(DEV), keep_traj=True, cache_branch=k, **kw)
    finally:
        eng.max_batch_override = None
    torch.testing.assert_close(tr2, traj, rtol=1e-5, atol=3e-6)
    eng.check()


# ---- 6. DDPM ------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ddpm_net(cin):
    from tests.test_gpu_unet import _tiny

    return _tiny(cin, 3, 1010 + cin, "fp32")   # (cfg, net, sd)


def _ddpm_inputs(Bn=B2):
    xT = randn(7601, Bn, 3, 16, 16)
    cond = (randn(7602, Bn, 3, 16, 16) * 0.5).clamp(-1, 1)
    cond[:, :, 4:10, 5:11] = -2.0
    return xT, cond


@pytest.mark.parametrize("mode", ["prior", "amortized", "amortized_corr1", "ddim"])
def test_cached_ddpm_vs_restatement(mode):
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, Replacement
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib

    ddpm = DDPM(25)
    K, k = ddpm.Ns, 2
    T = {n: v.numpy() for n, v in ddpm.host_tables().items()}
    xT, cond = _ddpm_inputs()
    nc = int(mode.endswith("corr1"))
    cin = 3 if mode == "prior" else 6
    cfg, net, sd = _ddpm_net(cin)
    n_evals = K * (1 + nc)
    full = R.interval_schedule(n_evals, 2)
    draws = [randn(7700 + j, B2, 3, 16, 16) for j in range(3 * K)]
    eps = R.cached_eps(sd, cfg, ddpm.time, k, full)
    lik = InPainting(patch_size=6, pad_value=-2)
    fc = sampling.FeatureCache(interval=2, branch=k)
    fast = sampling.make_eps_model(net, ddpm)
    if mode == "prior":
        ref, used, n_eval = DR.sample(eps, T, xT, draws, mode="prior")
        run = lambda c: sampling.get_prior_sample_fn(fast, ddpm, Replacement(0.1, 1.0, True, 0), lik, feature_cache=c)(xT.to(DEV))   # noqa: E731
        ekw = dict(mode=_lib.DDPM_PRIOR)
    elif mode.startswith("amortized"):
        ref, used, n_eval = DR.sample(eps, T, xT, draws, mode="amortized", cond=cond, amortized=True, n_corrector=nc, delta=0.1, tmin=ddpm.tmin,
                                      tmax=ddpm.tmax)
        run = lambda c: sampling.get_conditional_sample_fn(fast, ddpm, Amortized(0.9, nc, 0.1), lik, feature_cache=c)(xT.to(DEV), cond.to(DEV))   # noqa: E731
        ekw = dict(mode=_lib.DDPM_AMORTIZED, cond=cond.to(DEV), n_corrector=nc, delta=0.1)
    else:
        ref, used, n_eval = DR.sample(eps, T, xT, draws, mode="ddim", cond=cond, amortized=True)
        run = lambda c: sampling.get_ddim_sample_fn(fast, ddpm.with_feature_cache(c), lik)(xT.to(DEV), cond.to(DEV))   # noqa: E731
        ekw = dict(mode=_lib.DDIM, cond=cond.to(DEV))
    assert n_eval == n_evals == eps.net.e
    with sampling.injected_noise(draws):
        got = run(fc).cpu()
    with sampling.injected_noise(draws):
        plain = run(None).cpu()
    _report(f"{mode}: cached DDPM vs fp64 restatement", got, ref)
    print(f"   (the schedule moves the result by {float((got - plain).abs().max()):.3e})")
    assert float((got - plain).abs().max()) > 1e-3
    torch.testing.assert_close(got.double(), ref, **SAMPLER_TOL)
    # all-full is the uncached loop, bit for bit (injected and device noise)
    eng = net.engine(DEV)
    noise = torch.stack(draws).to(DEV)
    for nz in (dict(noise=noise), dict(seed=4242)):
        a = eng.ddpm_sample(xT.to(DEV).clone(), ddpm.host_tables(), tmin=ddpm.tmin, tmax=ddpm.tmax, **ekw, **nz)
        b = eng.ddpm_sample(xT.to(DEV).clone(), ddpm.host_tables(), tmin=ddpm.tmin, tmax=ddpm.tmax, cache_interval=1, cache_branch=k, **ekw, **nz)
        assert torch.equal(a, b), (mode, list(nz))
    eng.check()


def test_cached_repaint_walk_with_upward_moves():
    from image_diffusion.conditioning import repaint_walk
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib

    r = DDPM(100).respace(6)
    K, sf, k = 6, 0.5, 2
    T = {n: v.numpy() for n, v in r.host_tables().items()}
    xT, cond = _ddpm_inputs()
    walk = repaint_walk(K, 2, 2)
    n_down = sum(1 for a, b in zip(walk, walk[1:]) if b < a)
    assert n_down == 10 and len(walk) - 1 - n_down == 4
    full = R.interval_schedule(n_down, 2)
    cfg, net, sd = _ddpm_net(3)
    draws = [randn(7800 + j, B2, 3, 16, 16) for j in range(3 * K + 8)]
    eps = R.cached_eps(sd, cfg, r.time, k, full)
    ref, used, n_eval = DR.sample(eps, T, xT, draws, mode="replacement", cond=cond, start_fraction=sf, noise_condition=True,
                                  walk=DR.repaint_levels(K, 2, 2))
    assert n_eval == n_down
    eng = net.engine(DEV)
    kw = dict(mode=_lib.DDPM_REPLACEMENT, cond=cond.to(DEV), noise=torch.stack(draws[:used]).to(DEV), start_fraction=sf, noise_condition=True,
              tmin=r.tmin, tmax=r.tmax, timesteps=r.timesteps, train_steps=r.base_Ns, walk=walk)
    got = eng.ddpm_sample(xT.to(DEV).clone(), r.host_tables(), cache_interval=2, cache_branch=k, **kw).cpu()
    plain = eng.ddpm_sample(xT.to(DEV).clone(), r.host_tables(), **kw).cpu()
    allfull = eng.ddpm_sample(xT.to(DEV).clone(), r.host_tables(), cache_schedule=[1] * n_down, cache_branch=k, **kw).cpu()
    _report("RePaint walk: cached vs fp64 restatement", got, ref)
    assert torch.equal(plain, allfull) and float((got - plain).abs().max()) > 1e-3
    torch.testing.assert_close(got.double(), ref, **SAMPLER_TOL)
    eng.check()


# ---- 7. drift ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", [128, 64 * 8 * 8, 32 * 16 * 16 + 128])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_feature_drift_op_vs_fp64(dtype, per):
    from mi355 import _lib

    L = _lib.lib()
    Bn = 3
    tt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    code = {"fp32": _lib.MI355_F32, "bf16": _lib.MI355_BF16, "fp16": _lib.MI355_F16}[dtype]
    cur = (randn(900 + per % 97, Bn, per) * 1.5).to(tt)
    prev = (cur.float() + randn(901 + per % 97, Bn, per) * torch.tensor([0.05, 0.5, 2.0])[:, None]).to(tt)
    want = R.drift(cur, prev)                      # fp64 of the rounded inputs
    guard = 64
    bufs = []
    for t in (cur, prev):
        b = torch.full((t.numel() + 2 * guard,), 7.0, dtype=tt, device=DEV)
        b[guard:guard + t.numel()] = t.flatten().to(DEV)
        bufs.append(b)
    out = torch.full((Bn + 2,), -5.0, device=DEV)
    pc, pp = bufs[0][guard:], bufs[1][guard:]
    rc = L.mi355_feature_drift(C.c_void_p(pc.data_ptr()), C.c_void_p(pp.data_ptr()), code, Bn, per, C.c_void_p(out[1:].data_ptr()), None)
    assert rc == 0, L.mi355_last_error()
    torch.cuda.synchronize()
    got = out[1:1 + Bn].cpu().double()
    rel = float(((got - want).abs() / want).max())
    print(f"{dtype} per {per}: drift {[f'{v:.4e}' for v in want.tolist()]}, max relative error {rel:.2e}")
    assert rel < 1e-5
    assert out[0].item() == -5.0 and out[-1].item() == -5.0
    assert torch.equal(bufs[1][guard:guard + cur.numel()].cpu(), cur.flatten())            # prev <- cur
    assert torch.equal(bufs[0][guard:guard + cur.numel()].cpu(), cur.flatten())            # cur untouched
    for b in bufs:
        assert bool((b[:guard] == 7.0).all()) and bool((b[guard + cur.numel():] == 7.0).all()), "a guard band was written"
    # refusals: a tail that is no whole 16-byte fragment, a misaligned buffer, cur == prev
    assert L.mi355_feature_drift(C.c_void_p(pc.data_ptr()), C.c_void_p(pp.data_ptr()), code, Bn, per - 1, C.c_void_p(out.data_ptr()), None) == -2
    assert L.mi355_feature_drift(C.c_void_p(pc.data_ptr() + 4), C.c_void_p(pp.data_ptr()), code, 1, per // 2, C.c_void_p(out.data_ptr()), None) == -2
    assert L.mi355_feature_drift(C.c_void_p(pc.data_ptr()), C.c_void_p(pc.data_ptr()), code, Bn, per, C.c_void_p(out.data_ptr()), None) == -1


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sampler_drift_out(precision):
    idx, k = 0, 3
    eng = _net(idx, precision).engine(DEV)
    x0 = randn(1, B2, 3, 16, 16)
    tsp = torch.linspace(0, 1, N_STEPS + 1)
    kw = EULER_SCHEDULES["list"]
    full = _full_list(kw)
    _, ref_drift = R.cached_euler(tiny_sd(idx), TINY[idx], x0, tsp, k, full)
    x, traj, _, drift = eng.cfm_euler(x0.to(DEV), tsp.tolist(), keep_traj=True, cache_branch=k, cache_drift=True, **kw)
    x2, traj2, _ = eng.cfm_euler(x0.to(DEV), tsp.tolist(), keep_traj=True, cache_branch=k, **kw)
    assert torch.equal(traj, traj2)   # measuring changes nothing
    drift = drift.cpu().double()
    print(f"{precision}: drift rows\n{drift}\nrestatement\n{ref_drift}")
    assert tuple(drift.shape) == (N_STEPS, B2)
    meas = torch.tensor([bool(f) for f in full]) & (torch.arange(N_STEPS) > 0)
    assert bool((drift[~meas] == -1).all()) and bool((ref_drift[~meas] == -1).all()) and int(meas.sum()) == 2
    # With both features within delta * ||F|| of the restatement's (delta: the relative part of the bound the state and the forward are held to,
    # 5e-4 in fp32 - test_cached_euler - and 0.02 in bf16, the forward's relative rms), ||F_e - F_prev|| is within 2 delta ||F|| of its own, i.e.
    # within 2 delta / sqrt(drift) relatively, and the squared norm within twice that; the denominator's 2 delta is small beside it.
    delta = 5e-4 if precision == "fp32" else 0.02
    rel = (drift[meas] - ref_drift[meas]).abs() / ref_drift[meas]
    bound = 4 * delta / ref_drift[meas].sqrt() + 2 * delta
    print(f"relative error {rel.tolist()} against bounds {bound.tolist()}")
    assert bool((rel <= bound).all())
    # every step measured: the tool's schedule
    _, _, _, d1 = eng.cfm_euler(x0.to(DEV), tsp.tolist(), cache_interval=1, cache_branch=k, cache_drift=True)
    assert bool((d1[0] == -1).all()) and bool((d1[1:] > 0).all())
    eng.check()


# ---- 8. refusals through the C ABI -----------------------------------------------------------------------------------------------------------------

def test_cache_refusals():
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib
    from tests.test_gpu_unet import build

    L = _lib.lib()
    eng = _net(0, "fp32").engine(DEV)
    x0 = randn(1, B2, 3, 16, 16).to(DEV)
    x = x0.clone()
    ts = (C.c_float * (N_STEPS + 1))(*torch.linspace(0, 1, N_STEPS + 1).tolist())
    ddpm = DDPM(6)
    tb, keep = eng._ddpm_tables(ddpm.host_tables())
    opt = _lib.DDPMOptionsC(_lib.DDPM_PRIOR, 1, 0.1, 1e-5, 1.0, 1.0, 1, -2.0, -2.0, 1, 0)
    sched = eng._ddpm_schedule(ddpm.host_tables(), list(range(6)), 6, None, None)
    ws, wsb = eng.workspace(B2)

    def euler(fc):
        return L.mi355_cfm_euler_sample_cached(eng.handle, C.c_void_p(x.data_ptr()), 3, None, 0, 0, None, ts, N_STEPS + 1, None, None, B2, ws, wsb, None,
                                               C.byref(fc) if fc is not None else None)

    def ddpm_call(fc):   # 6 steps, one corrector each: 12 evaluations
        return L.mi355_ddpm_sample_sched_cached(eng.handle, C.c_void_p(x.data_ptr()), 3, None, C.byref(tb), C.byref(opt), C.byref(sched[0]), None, 0, B2,
                                                ws, wsb, None, C.byref(fc) if fc is not None else None)

    def fc(branch=1, full=(1, 0, 1, 0, 1, 0), n=None, null_full=False):
        c = _lib.feature_cache(branch, full)
        if n is not None:
            c.n_evals = n
        if null_full:
            c.full = None
        return c

    for call, n_ok in ((euler, N_STEPS), (ddpm_call, 12)):
        ok = [1, 0] * (n_ok // 2)
        bad = [(None, "cache is null"), (fc(full=ok, null_full=True), "cache->full is null"), (fc(full=[0] + ok[1:]), "cache->full[0]"),
               (fc(full=ok + [1]), "cache->n_evals"), (fc(full=ok[:-1]), "cache->n_evals"), (fc(0, ok), "cache->branch"), (fc(4, ok), "cache->branch"),
               (fc(-1, ok), "cache->branch")]
        for c, msg in bad:
            assert call(c) == -1, msg
            assert msg.encode() in L.mi355_last_error(), (msg, L.mi355_last_error())
    # the forward: a bad branch, and a differentiable plan
    out = torch.empty_like(x0)
    t = torch.tensor([0.2, 0.7], device=DEV)

    def fwd(e, branch):
        w, wb = e.workspace(B2)
        return L.mi355_unet_forward_cached(e.handle, C.c_void_p(x.data_ptr()), 3, None, 0, C.c_void_p(t.data_ptr()), 0.0, None, C.c_void_p(out.data_ptr()),
                                           B2, w, wb, None, branch)

    for b in (-1, 4):
        assert fwd(eng, b) == -1 and b"branch" in L.mi355_last_error()
    deng = _net(0, "fp32").engine(DEV, differentiable=True)
    assert fwd(deng, 0) == 0
    assert fwd(deng, 1) == -4 and b"differentiable" in L.mi355_last_error()
    dws, dwsb = deng.workspace(B2)
    assert L.mi355_cfm_euler_sample_cached(deng.handle, C.c_void_p(x.data_ptr()), 3, None, 0, 0, None, ts, N_STEPS + 1, None, None, B2, dws, dwsb, None,
                                           C.byref(fc(full=[1, 0] * 3))) == -4
    assert L.mi355_feature_cache_workspace_bytes(eng.handle, B2, 9, 1) == -1 and b"branch" in L.mi355_last_error()
    base = L.mi355_unet_workspace_bytes(eng.handle, B2)
    assert L.mi355_feature_cache_workspace_bytes(eng.handle, B2, 3, 0) == (base + 255) // 256 * 256
    assert L.mi355_feature_cache_workspace_bytes(eng.handle, B2, 3, 1) == (base + 255) // 256 * 256 + B2 * 64 * 8 * 8 * 4
    torch.cuda.synchronize()
    assert torch.equal(x, x0)   # nothing was launched: the state is untouched
    # the same calls with a valid schedule run
    assert euler(fc(full=[1, 0] * 3)) == 0 and ddpm_call(fc(2, [1, 0] * 6)) == 0
    torch.cuda.synchronize()
    assert not torch.equal(x, x0)
    eng.check()
    del keep
