"""CPU: feature reuse across sampler steps (DeepCache) - the restatement's own properties (tests/feature_cache_ref.py: a shallow evaluation on
the feature of the same input IS the full forward; on another input's feature it is far from both forwards, so a GPU path that ignored the cache
or recomputed everything would be far outside any tolerance), mi355_unet_cache_info against oracle.unet_ref.build_plan, schedule validation and
the Python refusals (before any device work).
"""
import ctypes as C
import functools

import pytest
import torch

from mi355.synth import randn, synth_state_dict
from oracle import unet_ref
from oracle.unet_ref import UNetConfig
from tests import feature_cache_ref as R

TINY = (UNetConfig(16, 3, 32, 3, 1, (2,), channel_mult=(1, 2), num_heads=2),
        UNetConfig(16, 3, 32, 3, 1, (2,), channel_mult=(1, 2), num_heads=2, use_scale_shift_norm=True, resblock_updown=True))
CIFAR = UNetConfig(32, 3, 128, 3, 2, (2,), channel_mult=(1, 2, 2, 2), num_heads=4, num_head_channels=64)


@functools.lru_cache(maxsize=None)
def tiny_sd(idx):
    from image_diffusion.unet import param_shapes

    return synth_state_dict(param_shapes(TINY[idx]), 1003)


def tiny_inputs():
    """(x0, t0, x1, t1): two independent inputs at B = 2."""
    return randn(1, 2, 3, 16, 16), torch.tensor([0.2, 0.7]), randn(2, 2, 3, 16, 16), torch.tensor([0.5, 0.9])


def _config_c(cfg, **kw):
    from mi355 import _lib

    return _lib.make_config(image_size=cfg.image_size, in_channels=cfg.in_channels, model_channels=cfg.model_channels, out_channels=cfg.out_channels,
                            num_res_blocks=cfg.num_res_blocks, attention_ds=cfg.attention_resolutions, channel_mult=cfg.channel_mult,
                            conv_resample=cfg.conv_resample, num_heads=cfg.num_heads, num_head_channels=cfg.num_head_channels,
                            use_scale_shift_norm=cfg.use_scale_shift_norm, resblock_updown=cfg.resblock_updown,
                            use_new_attention_order=cfg.use_new_attention_order, **kw)


def _cache_info(cfg, branch):
    from mi355 import _lib

    buf = (C.c_int32 * 8)()
    c = _config_c(cfg)
    rc = _lib.lib().mi355_unet_cache_info(C.byref(c), branch, buf)
    return rc, list(buf)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("idx", [0, 1])
def test_restatement_identity_and_sensitivity(idx, k):
    sd, cfg = tiny_sd(idx), TINY[idx]
    x0, t0, x1, t1 = tiny_inputs()
    y0, y1 = unet_ref.unet_forward(sd, cfg, x0, t0), unet_ref.unet_forward(sd, cfg, x1, t1)
    yf, feat = R.full_with_feature(sd, cfg, x0, t0, k)
    assert torch.equal(yf, y0)
    assert torch.equal(R.shallow(sd, cfg, x0, t0, k, feat), y0)   # the same layers on the same values
    mixed = R.shallow(sd, cfg, x1, t1, k, feat)
    d1, d0 = float((mixed - y1).abs().max()), float((mixed - y0).abs().max())
    print(f"net {idx} branch {k}: shallow(x1 | F(x0)) differs from full(x1) by {d1:.2f}, from full(x0) by {d0:.2f} (scale {float(y0.abs().max()):.2f})")
    assert d1 > 0.1 and d0 > 0.1


def test_restatement_loops():
    """All-full schedules are the oracle's own loops; the drift rows are -1 except at the full evaluations after the first."""
    from oracle import cfm_ref

    sd, cfg = tiny_sd(0), TINY[0]
    x0 = randn(1, 2, 3, 16, 16)
    ts = torch.linspace(0, 1, 5)
    traj, drift = R.cached_euler(sd, cfg, x0, ts, 2, [True] * 4)
    want = cfm_ref.euler_trajectory(unet_ref.model_fn(sd, cfg), x0, ts)
    torch.testing.assert_close(traj.float(), want, rtol=1e-5, atol=1e-6)
    assert bool((drift[0] == -1).all()) and bool((drift[1:] > 0).all())
    traj2, drift2 = R.cached_euler(sd, cfg, x0, ts, 2, [True, False, True, False])
    assert torch.equal(traj2[1], traj[1]) and float((traj2[-1] - traj[-1]).abs().max()) > 1e-3
    assert bool((drift2[[0, 1, 3]] == -1).all()) and bool((drift2[2] > 0).all())
    a, b = randn(3, 2, 5, 4, 4), randn(4, 2, 5, 4, 4)
    torch.testing.assert_close(R.drift(a, b), ((a - b).double() ** 2).sum((1, 2, 3)) / (b.double() ** 2).sum((1, 2, 3)))


def _flops(layers, hw, mc):
    """conv + attention 2 * MACs of a block at `hw` pixels entering it -> (flops, pixels leaving it); emb_layers not counted (they are part of
    the prelude every evaluation pays)."""
    f = 0.0
    for layer in layers:
        kind = layer[0]
        if kind == "conv":
            f += 2.0 * hw * layer[2] * layer[1] * 9
        elif kind == "res":
            _, cin, cout, up, down = layer
            if up:
                hw *= 4
            if down:
                hw //= 4
            f += 2.0 * hw * cout * cin * 9 + 2.0 * hw * cout * cout * 9 + (2.0 * hw * cout * cin if cin != cout else 0.0)
        elif kind == "attn":
            c = layer[1]
            f += 2.0 * hw * 3 * c * c + 4.0 * hw * hw * c + 2.0 * hw * c * c
        elif kind == "down":
            hw //= 4
            f += 2.0 * hw * layer[1] * layer[1] * 9 if layer[2] else 0.0
        elif kind == "up":
            hw *= 4
            f += 2.0 * hw * layer[1] * layer[1] * 9 if layer[2] else 0.0
    return f, hw


def _plan_numbers(cfg):
    """Per branch k: (cached feature (C, H), retained share of the conv + attention FLOPs), from build_plan alone."""
    ib, mid, ob, input_ch = unet_ref.build_plan(cfg)
    n = len(ib)
    hw = cfg.image_size ** 2
    fi, fo, feat = [], [], []
    for layers in ib:
        f, hw = _flops(layers, hw, cfg.model_channels)
        fi.append(f)
    fm, hw = _flops(mid, hw, cfg.model_channels)
    ch = mid[-1][2]
    for layers in ob:
        feat.append((ch, int(round(hw ** 0.5))))
        f, hw = _flops(layers, hw, cfg.model_channels)
        fo.append(f)
        ch = layers[0][2]
    f_out = 2.0 * hw * cfg.out_channels * input_ch * 9
    mc = cfg.model_channels
    emb_total = sum((2 if cfg.use_scale_shift_norm else 1) * l[2] for blk in ib + [mid] + ob for l in blk if l[0] == "res")
    f_emb = 2.0 * 4 * mc * emb_total + 2.0 * mc * 4 * mc + 2.0 * 4 * mc * 4 * mc
    total = sum(fi) + fm + sum(fo) + f_out + f_emb
    return n, {k: (feat[n - k], 1.0 - (sum(fi[k:]) + fm + sum(fo[:n - k])) / total) for k in range(1, n)}


def test_cache_info_matches_build_plan():
    import __graft_entry__ as ge

    ge.build()
    rc, buf = _cache_info(CIFAR, 0)
    assert rc == 0 and buf == [11, 0, 0, 0, 0, 0, 0, 0]
    n, plan = _plan_numbers(CIFAR)
    assert n == 12
    res = {}
    for k in range(1, 12):
        rc, buf = _cache_info(CIFAR, k)
        assert rc == 0 and buf[0] == 11 and 0 < buf[1] < buf[2]
        (c, h), share = plan[k]
        assert (buf[4], buf[5], buf[6]) == (c, h, h), (k, buf)
        assert abs(buf[7] / 1e6 - share) < 2e-6, (k, buf[7], share)   # ppm rounding
        res[k] = buf[5]
    assert [res[k] for k in range(1, 12)] == [32] * 3 + [16] * 3 + [8] * 3 + [4] * 2
    rc, buf = _cache_info(CIFAR, 3)
    assert (buf[4], buf[5], buf[6]) == (256, 32, 32) and round(buf[7] / 1e6, 2) == 0.36
    assert round(_cache_info(CIFAR, 1)[1][7] / 1e6, 2) == 0.08
    # the skipped ranges nest: a deeper branch skips less
    ranges = [_cache_info(CIFAR, k)[1][1:3] for k in range(1, 12)]
    assert all(a[0] < b[0] and a[1] > b[1] for a, b in zip(ranges, ranges[1:]))
    for cfg in TINY:
        n, plan = _plan_numbers(cfg)
        assert n == 4 and _cache_info(cfg, 0)[1][0] == 3
        shapes = []
        for k in (1, 2, 3):
            rc, buf = _cache_info(cfg, k)
            assert rc == 0 and abs(buf[7] / 1e6 - plan[k][1]) < 2e-6
            shapes.append(tuple(buf[4:7]))
        assert shapes == [(32, 16, 16), (64, 16, 16), (64, 8, 8)]


def test_cache_info_and_host_side_refusals():
    from mi355 import _lib

    L = _lib.lib()
    for k in (-1, 12):
        rc, _ = _cache_info(CIFAR, k)
        assert rc == -1 and b"branch" in L.mi355_last_error()
    buf = (C.c_int32 * 8)()
    assert L.mi355_unet_cache_info(None, 1, buf) == -1
    c = _config_c(CIFAR)
    assert L.mi355_unet_cache_info(C.byref(c), 1, None) == -1
    # the entry points refuse a null handle before anything else
    assert L.mi355_unet_forward_cached(None, None, 3, None, 0, None, 0.0, None, None, 1, None, 0, None, 1) < 0
    assert L.mi355_cfm_euler_sample_cached(None, None, 3, None, 0, 0, None, None, 2, None, None, 1, None, 0, None, None) < 0
    assert L.mi355_ddpm_sample_sched_cached(None, None, 3, None, None, None, None, None, 0, 1, None, 0, None, None) < 0
    assert L.mi355_feature_cache_workspace_bytes(None, 1, 1, 0) < 0
    assert L.mi355_feature_drift(None, None, 0, 1, 128, None, None) == -1
    for name in ("mi355_unet_cache_info", "mi355_unet_forward_cached", "mi355_cfm_euler_sample_cached", "mi355_ddpm_sample_sched_cached",
                 "mi355_feature_cache_workspace_bytes", "mi355_feature_drift"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.mi355_version() == 108   # additive: new symbols only


def test_schedule_validation():
    from mi355._lib import feature_cache
    from mi355.engine import ddpm_eval_count, feature_cache_args as cache_schedule
    from mi355 import _lib

    assert cache_schedule(6) is None
    assert cache_schedule(6, interval=3) == (1, [True, False, False, True, False, False])
    assert cache_schedule(6, interval=1, branch=2) == (2, [True] * 6)
    assert cache_schedule(3, schedule=[1, 0, 2], branch=3) == (3, [True, False, True])
    assert cache_schedule(5, interval=3)[1] == R.interval_schedule(5, 3)
    with pytest.raises(ValueError, match="cache_interval and cache_schedule"):
        cache_schedule(6, interval=2, schedule=[1] * 6)
    with pytest.raises(ValueError, match="one entry per network evaluation"):
        cache_schedule(6, schedule=[1] * 5)
    with pytest.raises(ValueError, match=r"cache_schedule\[0\]"):
        cache_schedule(3, schedule=[0, 1, 1])
    with pytest.raises(ValueError, match="cache_interval"):
        cache_schedule(6, interval=0)
    with pytest.raises(ValueError, match="cache_branch"):
        cache_schedule(6, interval=2, branch=0)
    with pytest.raises(ValueError, match="needs a schedule"):
        cache_schedule(6, branch=2)
    with pytest.raises(NotImplementedError, match="guided"):
        cache_schedule(6, interval=2, guidance_scale=2.0)
    fc = feature_cache(2, [1, 0, 1])
    assert (fc.branch, fc.n_evals, [fc.full[i] for i in range(3)], bool(fc.drift_out)) == (2, 3, [1, 0, 1], False)
    # evaluations in loop order: one per downward move, correctors behind each ancestral predictor, none in DDIM mode
    assert ddpm_eval_count(25, _lib.DDPM_PRIOR, 0) == 25 and ddpm_eval_count(25, _lib.DDPM_AMORTIZED, 1) == 50
    assert ddpm_eval_count(25, _lib.DDIM, 1) == 25
    assert ddpm_eval_count(6, _lib.DDPM_REPLACEMENT, 1, walk=[6, 5, 4, 5, 6, 5, 4, 3, 2, 1, 0]) == 16


def _fake_engine():
    """A UNetEngine without a handle: the host checks that run before any device work."""
    from mi355.engine import UNetEngine

    class Rec(UNetEngine):
        def __init__(self):
            self.device = torch.device("cpu")
            self.num_classes, self.in_channels, self.out_channels, self.image_size = 0, 3, 3, 16
            self.max_batch_override = None

        def __del__(self):
            pass

    return Rec()


def test_python_refusals():
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, ClassifierFreeGuidance, ReconstructionGuidance
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib
    from torchcfm_compat import NeuralODE, UNetModelWrapper

    eng = _fake_engine()
    x = torch.zeros(2, 3, 16, 16)
    ts = [0.0, 0.5, 1.0]
    with pytest.raises(ValueError, match="cache_interval and cache_schedule"):
        eng.cfm_euler(x, ts, cache_interval=2, cache_schedule=[1, 0])
    with pytest.raises(NotImplementedError, match="guided.*Runge-Kutta.*multistep.*shaped.*reconstruction.*SF2M"):
        eng.cfm_euler(x, ts, cond=x, guidance_scale=2.0, cache_interval=2)
    with pytest.raises(ValueError, match="one entry per network evaluation"):
        eng.cfm_euler(x, ts, cache_schedule=[1, 0, 0])
    with pytest.raises(ValueError, match="cache_drift"):
        eng.cfm_euler(x, ts, cache_drift=True)
    T = DDPM(6).host_tables()
    with pytest.raises(ValueError, match="cache_interval and cache_schedule"):
        eng.ddpm_sample(x, T, mode=_lib.DDPM_PRIOR, cache_interval=2, cache_schedule=[1] * 6)
    with pytest.raises(NotImplementedError, match="guided"):
        eng.ddpm_sample(x, T, mode=_lib.DDPM_AMORTIZED, cond=x, guidance_scale=2.0, cache_interval=2)
    with pytest.raises(ValueError, match="one entry per network evaluation"):
        eng.ddpm_sample(x, T, mode=_lib.DDPM_PRIOR, n_corrector=1, cache_schedule=[1] * 6)   # 12 evaluations
    # the sampling front end
    with pytest.raises(ValueError):
        sampling.FeatureCache()
    with pytest.raises(ValueError):
        sampling.FeatureCache(interval=2, schedule=[1, 0])
    fc = sampling.FeatureCache(interval=3, branch=2)
    assert fc.kwargs() == dict(cache_interval=3, cache_schedule=None, cache_branch=2)
    assert sampling.FeatureCache(schedule=[1, 0]).kwargs() == dict(cache_interval=None, cache_schedule=(True, False), cache_branch=1)
    ddpm, lik = DDPM(6), InPainting(patch_size=6, pad_value=-2)
    eps = lambda x, t: x   # noqa: E731
    with pytest.raises(NotImplementedError, match="ClassifierFreeGuidance"):
        sampling.get_conditional_sample_fn(eps, ddpm, ClassifierFreeGuidance(0.9, 0, 0.1, 2.0), lik, feature_cache=fc)
    with pytest.raises(NotImplementedError, match="ReconstructionGuidance"):
        sampling.get_conditional_sample_fn(eps, ddpm, ReconstructionGuidance(1.0, 0.5, "before", 0, 0.1), lik, feature_cache=fc)
    # the chain carries it to the sample functions whose signatures are fixed; it commutes with respace and with x0 shaping
    cached = ddpm.with_feature_cache(fc)
    assert cached.feature_cache is fc and ddpm.feature_cache is None and DDPM(25).with_feature_cache(fc).respace(5).feature_cache is fc
    assert cached.with_x0_shaping(0.9, 2.0).feature_cache is fc and cached.with_feature_cache(None).feature_cache is None
    with pytest.raises(NotImplementedError, match="DPM-Solver"):
        sampling.get_dpm_solver_sample_fn(eps, cached, lik)
    with pytest.raises(NotImplementedError, match="guided"):
        sampling.get_ddim_sample_fn(eps, cached, lik, guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="ClassifierFreeGuidance"):
        sampling.get_conditional_sample_fn(eps, cached, ClassifierFreeGuidance(0.9, 0, 0.1, 2.0), lik)
    with pytest.raises(NotImplementedError, match="fused loop"):
        sampling.get_ddim_sample_fn(eps, cached, lik)(x, x)
    with pytest.raises(NotImplementedError, match="fused loop"):   # an arbitrary callable has no plan to cut
        sampling.get_conditional_sample_fn(eps, ddpm, Amortized(0.9, 0, 0.1), lik, feature_cache=fc)(x, x)
    # the torchcfm front end: Euler on the wrapper only
    net = UNetModelWrapper(dim=(3, 16, 16), num_channels=32, num_res_blocks=1, channel_mult=(1, 2), num_heads=2, attention_resolutions="8")
    assert NeuralODE(net, solver="euler", cache_interval=3, cache_branch=2).cache == dict(cache_interval=3, cache_branch=2)
    assert NeuralODE(net, solver="euler").cache == {}
    with pytest.raises(NotImplementedError, match="euler"):
        NeuralODE(net, solver="rk4", cache_interval=3)
    with pytest.raises(NotImplementedError, match="UNetModelWrapper"):
        NeuralODE(lambda t, x: x, solver="euler", cache_interval=3)


def test_compute_fid_cache_flags():
    import compute_fid

    with pytest.raises(NotImplementedError, match="euler"):
        compute_fid.make_gen_1_img(None, integration_method="dopri5", cache_interval=3)
    with pytest.raises(NotImplementedError, match="euler"):
        compute_fid.make_gen_1_img(None, integration_method="rk4", cache_branch=2)
