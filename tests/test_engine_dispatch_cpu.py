"""CPU: what every public sampler of UNetEngine hands to the library - the entry points it calls and in which order, the batch, the Philox seed,
the rows of labels and per-image guidance scales and the number of injected draws of every call, and the arguments of the workspace size
functions it asks.  The engine is the real one without a handle (the pattern of tests/test_cfg_cpu.py, the seam one level lower): its library
is a recorder that reads those values back out of the ctypes arguments and structs at the moment of the call.

The expected values are the engine's behaviour when this file was written; a change of the marshalling code must leave every row as it is.
"""
import ctypes as C

import pytest
import torch

B, S, K = 3, 8, 4   # batch, image size, DDPM steps
SPAN = [0.0, 0.5, 1.0]
WS_BYTES = 64

# entry point -> where its arguments sit (the handle is argument 0): B the batch, lab the labels, wt the per-image scales, seed the scalar Philox
# seed, opt the options struct that carries the seed, nd the number of injected draws
POS = {
    "mi355_unet_forward": dict(B=7), "mi355_unet_forward_t": dict(B=7), "mi355_unet_forward_labels": dict(lab=7, B=9),
    "mi355_unet_forward_cached": dict(lab=7, B=9), "mi355_unet_forward_tiled": dict(lab=6, B=8),
    "mi355_cfm_euler_sample": dict(B=10), "mi355_cfm_euler_sample_labels": dict(lab=6, B=11), "mi355_cfm_euler_sample_cached": dict(lab=6, B=11),
    "mi355_cfm_euler_sample_tiled": dict(lab=6, B=11), "mi355_cfm_rk_sample": dict(lab=5, B=14), "mi355_cfm_cfg_sample": dict(lab=6, wt=9, B=18),
    "mi355_cfm_ab_sample": dict(lab=5, B=16), "mi355_cfm_ab_cfg_sample": dict(lab=6, wt=9, B=20),
    "mi355_cfm_recon_sample": dict(lab=3, seed=15, B=19), "mi355_sf2m_euler_sample": dict(lab=4, seed=10, B=15),
    "mi355_ddpm_sample": dict(opt=5, nd=7, B=8), "mi355_ddpm_sample_sched": dict(opt=5, nd=8, B=9),
    "mi355_ddpm_sample_sched_cached": dict(opt=5, nd=8, B=9), "mi355_ddpm_sample_tiled": dict(opt=5, nd=8, B=9),
    "mi355_ddpm_cfg_sample": dict(lab=4, wt=7, opt=9, nd=11, B=12), "mi355_ddpm_cfg_sample_sched": dict(lab=4, wt=7, opt=9, nd=12, B=13),
    "mi355_ddpm_multistep_sample": dict(opt=5, B=7), "mi355_ddpm_multistep_cfg_sample": dict(lab=4, wt=7, opt=9, B=11),
    "mi355_ddpm_shaped_sample": dict(lab=4, wt=8, opt=10, nd=15, B=16), "mi355_ddpm_lv_sample": dict(lab=4, wt=8, opt=10, nd=15, B=16),
    "mi355_ddpm_pred_sample": dict(lab=4, wt=8, opt=10, nd=17, B=18),
    "mi355_ddpm_vlb": dict(lab=4, opt=6, nd=8, B=11), "mi355_ddpm_vlb_pred": dict(lab=4, opt=6, nd=9, B=12),
}


def _plain(a):
    """A workspace-function argument as a plain value: a struct passed by reference becomes the tuple of its fields."""
    obj = getattr(a, "_obj", None)
    return tuple(getattr(obj, f) for f, _ in obj._fields_) if isinstance(obj, C.Structure) else a


def _rows(p, n, ctype):
    return None if p is None or not p.value else list(C.cast(p, C.POINTER(ctype))[:n])


class Recorder:
    """Stands where the loaded library stands: every attribute is a function that records its call and returns 0 (a size function: WS_BYTES)."""

    def __init__(self):
        self.calls, self.sizes = [], []

    def __getattr__(self, name):
        def fn(*args):
            if name.endswith("_workspace_bytes"):
                self.sizes.append((name,) + tuple(_plain(a) for a in args[1:]))
                return WS_BYTES
            pos = POS[name]
            n = args[pos["B"]]
            seed = args[pos["seed"]] if "seed" in pos else args[pos["opt"]]._obj.seed if "opt" in pos else None
            self.calls.append(dict(name=name, B=n, seed=seed, opt=_plain(args[pos["opt"]]) if "opt" in pos else None, lab=_rows(args[pos["lab"]], n, C.c_int32) if "lab" in pos else None,
                                   wt=_rows(args[pos["wt"]], n, C.c_float) if "wt" in pos else None, nd=args[pos["nd"]] if "nd" in pos else None))
            return 0

        return fn


def fake_engine(in_ch=1, out_ch=1, max_batch=1000):
    from mi355.engine import UNetEngine

    class Fake(UNetEngine):
        def __init__(self):   # no device, no handle
            self.device = torch.device("cpu")
            self.handle = None
            self.precision, self.differentiable = "fp32", True
            self.num_classes, self.in_channels, self.out_channels, self.image_size = 10, in_ch, out_ch, S
            self.max_batch_override = max_batch
            self._ws, self._ws_bytes, self._fwd, self._full_state = None, {}, None, None
            self.L = Recorder()

        def __del__(self):
            pass

        def _stream(self):
            return None

        def _chk(self, t, name, dtype=torch.float32):   # the engine's own, without the refusal of host tensors
            if t.dtype != dtype or not t.is_contiguous():
                raise TypeError(f"{name} must be contiguous {dtype}")
            return C.c_void_p(t.data_ptr())

    return Fake()


Y = [1, 4, 7]            # distinct per image, as are the scales
WT = [0.5, 1.5, 2.5]


class D:
    """Fresh operands of one row."""

    def __init__(self):
        g = torch.Generator().manual_seed(3)
        self.tables = {n: torch.rand(K, generator=g) + 0.1 for n in (
            "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2", "posterior_log_variance_clipped",
            "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "recip_sqrt_m1_alphas_cumprod", "alphas_cumprod_prev", "alphas", "betas")}
        self.y, self.wt = torch.tensor(Y), torch.tensor(WT)
        self.sched = dict(timesteps=[0, 2, 5, 7], train_steps=8)
        self.coefs = tuple(torch.rand(K, generator=g) for _ in range(3))
        self.logs = {n: torch.rand(K, generator=g) for n in ("true_log", "model_log", "min_log", "max_log")}
        self.vec = torch.rand(K, generator=g)   # a max_log / times / ddim_sigma row
        self.tiling = dict(stride=4, weight="tent", chunk=2)   # 12x12 canvases: 2 x 2 windows of 8x8, B * 4 windows in chunks of 2

    @staticmethod
    def x(c=1, hw=S):
        return torch.zeros(B, c, hw, hw)

    def noise(self, n, hw=S):
        return torch.zeros(n, B, 1, hw, hw)


def _lib():
    from mi355 import _lib as lib_

    return lib_


# row: (id, engine keywords, call(engine, operands))
ROWS = [
    ("forward", {}, lambda e, d: e.forward(d.x(), torch.zeros(B))),
    ("forward_host_t", {}, lambda e, d: e.forward(d.x(), 0.5)),
    ("forward_labels", dict(in_ch=2), lambda e, d: e.forward(d.x(), 0.5, cond=d.x(), y=d.y)),
    ("forward_cached", {}, lambda e, d: (e.forward_cached(d.x(), 0.5, branch=0), e.forward_cached(d.x(), 0.5, y=d.y, branch=1))),
    ("forward_tiled", dict(in_ch=2), lambda e, d: e.forward_tiled(d.x(1, 12), 0.5, cond=d.x(1, 12), y=d.y, tiling=d.tiling)),
    ("euler", {}, lambda e, d: e.cfm_euler(d.x(), SPAN, keep_traj=True, want_u8=True)),
    ("euler_labels", dict(in_ch=2), lambda e, d: e.cfm_euler(d.x(), SPAN, cond=d.x(), y=d.y, cond_drift=True)),
    ("euler_sliced", dict(in_ch=2, max_batch=2), lambda e, d: e.cfm_euler(d.x(), SPAN, cond=d.x(), y=d.y, keep_traj=True, want_u8=True)),
    ("euler_cached_interval", {}, lambda e, d: e.cfm_euler(d.x(), SPAN, cache_interval=2)),
    ("euler_cached_drift", {}, lambda e, d: e.cfm_euler(d.x(), SPAN, y=d.y, cache_schedule=[True, False], cache_branch=1, cache_drift=True)),
    ("euler_cached_drift_sliced", dict(max_batch=2),
     lambda e, d: e.cfm_euler(d.x(), SPAN, y=d.y, cache_schedule=[True, False], cache_drift=True, keep_traj=True, want_u8=True)),
    ("euler_tiled", {}, lambda e, d: e.cfm_euler(d.x(1, 12), SPAN, tiling=d.tiling, keep_traj=True, want_u8=True)),
    ("euler_tiled_labels_cond", dict(in_ch=2), lambda e, d: e.cfm_euler(d.x(1, 12), SPAN, cond=d.x(1, 12), y=d.y, tiling=d.tiling)),
    ("euler_guided", dict(max_batch=4), lambda e, d: e.cfm_euler(d.x(), SPAN, y=d.y, guidance_scale=d.wt, keep_traj=True, want_u8=True)),
    ("rk", {}, lambda e, d: e.cfm_rk(d.x(), SPAN, "rk4", keep_traj=True, want_u8=True)),
    ("rk_sliced", dict(in_ch=2, max_batch=2), lambda e, d: e.cfm_rk(d.x(), SPAN, "heun2", cond=d.x(), y=d.y, keep_traj=True, want_u8=True)),
    ("rk_guided_sliced", dict(max_batch=2), lambda e, d: e.cfm_rk(d.x(), SPAN, "midpoint", y=d.y, guidance_scale=d.wt, null_label=0)),
    ("cfg", dict(in_ch=2), lambda e, d: e.cfm_cfg(d.x(), SPAN, "rk4", cond=d.x(), guidance_scale=2.0)),
    ("ab", {}, lambda e, d: e.cfm_ab(d.x(), SPAN, "ab2", y=d.y)),
    ("ab_guided", dict(in_ch=2), lambda e, d: e.cfm_ab(d.x(), SPAN, "ab3", cond=d.x(), y=d.y, guidance_scale=d.wt)),
    ("ab_sliced", dict(max_batch=2), lambda e, d: e.cfm_ab(d.x(), SPAN, "ab2", y=d.y, keep_traj=True, want_u8=True)),
    ("ab_guided_sliced", dict(in_ch=2, max_batch=4),
     lambda e, d: e.cfm_ab(d.x(), SPAN, "ab3", cond=d.x(), y=d.y, guidance_scale=d.wt, keep_traj=True, want_u8=True)),
    ("recon", {}, lambda e, d: e.cfm_recon(d.x(), SPAN, d.x(), 0, replace="coupled", y_labels=d.y)),
    ("recon_fresh_philox_sliced", dict(max_batch=2),
     lambda e, d: e.cfm_recon(d.x(), SPAN, d.x(), 0, replace="fresh", seed=2 ** 64 - 1, final_paste=True, keep_traj=True, want_u8=True, y_labels=d.y)),
    ("recon_injected_loss_sliced", dict(max_batch=2),
     lambda e, d: e.cfm_recon(d.x(), SPAN, torch.zeros(B, 1, 4, 4), 2, scales=[0.5, 0.0], replace="fresh", noise=d.noise(2), return_loss=True)),
    ("sf2m", {}, lambda e, d: e.sf2m_euler(fake_engine(), d.x(), SPAN, 0.3, y=d.y, seed=77, outputs=[(0, 0.5)])),
    ("sf2m_sliced", dict(max_batch=2), lambda e, d: e.sf2m_euler(fake_engine(), d.x(), SPAN, 0.3, reverse=True, y=d.y, seed=77, outputs=[(0, 0.5)])),
    ("sf2m_injected_sliced", dict(max_batch=2), lambda e, d: e.sf2m_euler(fake_engine(), d.x(), SPAN, 0.3, dW=d.noise(2))),
    ("ddpm", {}, lambda e, d: e.ddpm_sample(d.x(), d.tables, mode=_lib().DDPM_PRIOR, noise=d.noise(5), seed=9)),
    ("ddpm_unguided_is_not_sliced", dict(in_ch=2, max_batch=2),
     lambda e, d: e.ddpm_sample(d.x(), d.tables, mode=_lib().DDPM_AMORTIZED, cond=d.x(), n_corrector=1, seed=9)),
    ("ddpm_sched", {}, lambda e, d: e.ddpm_sample(d.x(), d.tables, mode=_lib().DDIM, ddim_sigma=d.vec, noise=d.noise(4), seed=9, **d.sched)),
    ("ddpm_walk", dict(in_ch=1), lambda e, d: e.ddpm_sample(d.x(), d.tables, mode=_lib().DDPM_REPLACEMENT, cond=d.x(), walk=[4, 3, 4, 3, 2, 1, 0], **d.sched)),
    ("ddpm_cached", {}, lambda e, d: e.ddpm_sample(d.x(), d.tables, mode=_lib().DDPM_PRIOR, cache_interval=2, seed=9)),
    ("ddpm_cached_sched", {}, lambda e, d: e.ddpm_sample(d.x(), d.tables, mode=_lib().DDPM_PRIOR, n_corrector=1, cache_interval=3, cache_branch=1, **d.sched)),
    ("ddpm_tiled", dict(in_ch=2),
     lambda e, d: e.ddpm_sample(d.x(1, 12), d.tables, mode=_lib().DDPM_AMORTIZED, cond=d.x(1, 12), noise=d.noise(4, 12), tiling=d.tiling, seed=9)),
    ("ddpm_tiled_sched", {}, lambda e, d: e.ddpm_sample(d.x(1, 12), d.tables, mode=_lib().DDIM, tiling=d.tiling, **d.sched)),
    ("ddpm_guided", dict(in_ch=2),
     lambda e, d: e.ddpm_sample(d.x(), d.tables, mode=_lib().DDPM_AMORTIZED, cond=d.x(), noise=d.noise(4), guidance_scale=2.0, y=d.y, seed=9)),
    ("ddpm_guided_sched_sliced", dict(in_ch=2, max_batch=4),
     lambda e, d: e.ddpm_sample(d.x(), d.tables, mode=_lib().DDIM, cond=d.x(), guidance_scale=d.wt, y=d.y, seed=2 ** 64 - 1, ddim_sigma=d.vec,
                                start_fraction=0.5, noise_condition=False, pad_value=0.0, **d.sched)),
    ("ddpm_guided_injected_sliced", dict(in_ch=2, max_batch=2),
     lambda e, d: e.ddpm_sample(d.x(), d.tables, mode=_lib().DDPM_AMORTIZED, cond=d.x(), noise=d.noise(4), guidance_scale=d.wt, seed=9)),
    ("ddpm_prediction_v", {}, lambda e, d: e.ddpm_sample(d.x(), d.tables, mode=_lib().DDPM_PRIOR, prediction="v", seed=9)),
    ("multistep", {}, lambda e, d: e.ddpm_multistep(d.x(), d.tables, d.coefs)),
    ("multistep_unguided_is_not_sliced", dict(max_batch=2), lambda e, d: e.ddpm_multistep(d.x(), d.tables, d.coefs, **d.sched)),
    ("multistep_guided_sliced", dict(in_ch=2, max_batch=4),
     lambda e, d: e.ddpm_multistep(d.x(), d.tables, d.coefs, cond=d.x(), guidance_scale=d.wt, y=d.y, null_label=3, **d.sched)),
    ("shaped", {}, lambda e, d: e.ddpm_shaped(d.x(), d.tables, (0.9, 0.0, 0.0), mode=_lib().DDPM_PRIOR, noise=d.noise(4), seed=9)),
    ("shaped_unguided_is_one_call", dict(max_batch=2), lambda e, d: e.ddpm_shaped(d.x(), d.tables, None, mode=_lib().DDPM_PRIOR, seed=9, **d.sched)),
    ("shaped_multistep_guided_sliced", dict(in_ch=2, max_batch=4),
     lambda e, d: e.ddpm_shaped(d.x(), d.tables, (0.9, 0.0, 0.7), mode=_lib().DDIM, coefs=d.coefs, cond=d.x(), guidance_scale=d.wt, y=d.y, seed=9)),
    ("learned", dict(out_ch=2), lambda e, d: e.ddpm_learned(d.x(), d.tables, d.vec, mode=_lib().DDPM_PRIOR, noise=d.noise(4), seed=9)),
    ("learned_guided_sliced", dict(in_ch=2, out_ch=2, max_batch=4),
     lambda e, d: e.ddpm_learned(d.x(), d.tables, d.vec, mode=_lib().DDPM_AMORTIZED, cond=d.x(), noise=d.noise(4), guidance_scale=d.wt, seed=9)),
    ("learned_multistep", dict(out_ch=2), lambda e, d: e.ddpm_learned(d.x(), d.tables, d.vec, mode=_lib().DDIM, coefs=d.coefs)),
    ("learned_times_only", {}, lambda e, d: e.ddpm_learned(d.x(), d.tables, None, mode=_lib().DDPM_PRIOR, times=d.vec, seed=9)),
    ("pred_x0", {}, lambda e, d: e.ddpm_pred(d.x(), d.tables, "x0", mode=_lib().DDPM_PRIOR, noise=d.noise(4), seed=9)),
    ("pred_v_guided_shaped_sliced", dict(in_ch=2, max_batch=4),
     lambda e, d: e.ddpm_pred(d.x(), d.tables, "v", mode=_lib().DDIM, shaping=(0.9, 0.0, 0.7), cond=d.x(), guidance_scale=d.wt, y=d.y, seed=9)),
    ("pred_x0_multistep", {}, lambda e, d: e.ddpm_pred(d.x(), d.tables, "x0", mode=_lib().DDIM, coefs=d.coefs, **d.sched)),
    ("vlb_fixed_injected", {}, lambda e, d: e.ddpm_vlb(d.x(), d.tables, d.logs, learned=False, noise=d.noise(K))),
    ("vlb_learned_philox", dict(in_ch=2, out_ch=2), lambda e, d: e.ddpm_vlb(d.x(), d.tables, d.logs, learned=True, times=d.vec, cond=d.x(), y=d.y, seed=5)),
    ("vlb_pred_x0", {}, lambda e, d: e.ddpm_vlb(d.x(), d.tables, d.logs, learned=False, prediction="x0")),
    ("vlb_philox_sliced", dict(max_batch=2), lambda e, d: e.ddpm_vlb(d.x(), d.tables, d.logs, learned=False, y=d.y, seed=2 ** 64 - 1)),
    ("vlb_injected_sliced", dict(max_batch=2), lambda e, d: e.ddpm_vlb(d.x(), d.tables, d.logs, learned=False, noise=d.noise(K), prediction="v")),
]

TILE = (12, 12, 4, 4, 1, 2)   # the mi355_tile_plan of D.tiling
M64 = 2 ** 64 - 1

# id -> (entry points in call order, batches, seeds, calls that carry labels?, calls that carry per-image scales?, n_noise_draws, size-function calls)
EXPECT = {
    "forward": (["unet_forward"], [3], [None], [False], [False], [None], [("unet", 3)]),
    "forward_host_t": (["unet_forward_t"], [3], [None], [False], [False], [None], [("unet", 3)]),
    "forward_labels": (["unet_forward_labels"], [3], [None], [True], [False], [None], [("unet", 3)]),
    "forward_cached": (["unet_forward_cached"] * 2, [3, 3], [None, None], [False, True], [False, False], [None, None], [("unet", 3), ("unet", 3)]),
    "forward_tiled": (["unet_forward_tiled"], [3], [None], [True], [False], [None], [("tiled", 3, TILE)]),
    "euler": (["cfm_euler_sample"], [3], [None], [False], [False], [None], [("unet", 3)]),
    "euler_labels": (["cfm_euler_sample_labels"], [3], [None], [True], [False], [None], [("unet", 3)]),
    "euler_sliced": (["cfm_euler_sample_labels"] * 2, [2, 1], [None, None], [True, True], [False, False], [None, None], [("unet", 2), ("unet", 1)]),
    "euler_cached_interval": (["cfm_euler_sample_cached"], [3], [None], [False], [False], [None], [("unet", 3)]),
    "euler_cached_drift": (["cfm_euler_sample_cached"], [3], [None], [True], [False], [None], [("unet", 3), ("feature_cache", 3, 1, 1)]),
    "euler_cached_drift_sliced": (["cfm_euler_sample_cached"] * 2, [2, 1], [None, None], [True, True], [False, False], [None, None],
                                  [("unet", 2), ("feature_cache", 2, 1, 1), ("unet", 1), ("feature_cache", 1, 1, 1)]),
    "euler_tiled": (["cfm_euler_sample_tiled"], [3], [None], [False], [False], [None], [("tiled", 3, TILE)]),
    "euler_tiled_labels_cond": (["cfm_euler_sample_tiled"], [3], [None], [True], [False], [None], [("tiled", 3, TILE)]),
    "euler_guided": (["cfm_cfg_sample"] * 2, [2, 1], [None, None], [True, True], [True, True], [None, None], [("cfg", 2, 1), ("cfg", 1, 1)]),
    "rk": (["cfm_rk_sample"], [3], [None], [False], [False], [None], [("cfm_rk", 3, 4)]),
    "rk_sliced": (["cfm_rk_sample"] * 2, [2, 1], [None, None], [True, True], [False, False], [None, None], [("cfm_rk", 2, 2), ("cfm_rk", 1, 2)]),
    "rk_guided_sliced": (["cfm_cfg_sample"] * 3, [1, 1, 1], [None] * 3, [True] * 3, [True] * 3, [None] * 3, [("cfg", 1, 2)]),   # (sizes are cached)
    "cfg": (["cfm_cfg_sample"], [3], [None], [False], [False], [None], [("cfg", 3, 4)]),
    "ab": (["cfm_ab_sample"], [3], [None], [True], [False], [None], [("cfm_ab", 3, 2, 1, 0)]),
    "ab_guided": (["cfm_ab_cfg_sample"], [3], [None], [True], [True], [None], [("cfm_ab", 3, 3, 2, 1)]),
    "ab_sliced": (["cfm_ab_sample"] * 2, [2, 1], [None, None], [True, True], [False, False], [None, None],
                  [("cfm_ab", 2, 2, 1, 0), ("cfm_ab", 1, 2, 1, 0)]),
    "ab_guided_sliced": (["cfm_ab_cfg_sample"] * 2, [2, 1], [None, None], [True, True], [True, True], [None, None],
                         [("cfm_ab", 2, 3, 2, 1), ("cfm_ab", 1, 3, 2, 1)]),
    "recon": (["cfm_recon_sample"], [3], [0], [True], [False], [None], [("cfm_recon", 3, 0, 0)]),
    "recon_fresh_philox_sliced": (["cfm_recon_sample"] * 2, [2, 1], [M64, 0], [True, True], [False, False], [None, None],
                                  [("cfm_recon", 2, 0, 0), ("cfm_recon", 1, 0, 0)]),
    "recon_injected_loss_sliced": (["cfm_recon_sample"] * 2, [2, 1], [0, 1], [False, False], [False, False], [None, None],
                                   [("cfm_recon", 2, 4, 4), ("cfm_recon", 1, 4, 4)]),
    "sf2m": (["sf2m_euler_sample"], [3], [77], [True], [False], [None], [("unet", 3)]),
    "sf2m_sliced": (["sf2m_euler_sample"] * 2, [2, 1], [77, 78], [True, True], [False, False], [None, None], [("unet", 2), ("unet", 1)]),
    "sf2m_injected_sliced": (["sf2m_euler_sample"] * 2, [2, 1], [0, 0], [False, False], [False, False], [None, None], [("unet", 2), ("unet", 1)]),
    "ddpm": (["ddpm_sample"], [3], [9], [False], [False], [5], [("unet", 3)]),
    "ddpm_unguided_is_not_sliced": (["ddpm_sample"], [3], [9], [False], [False], [0], [("unet", 3)]),
    "ddpm_sched": (["ddpm_sample_sched"], [3], [9], [False], [False], [4], [("unet", 3)]),
    "ddpm_walk": (["ddpm_sample_sched"], [3], [0], [False], [False], [0], [("unet", 3)]),
    "ddpm_cached": (["ddpm_sample_sched_cached"], [3], [9], [False], [False], [0], [("unet", 3)]),
    "ddpm_cached_sched": (["ddpm_sample_sched_cached"], [3], [0], [False], [False], [0], [("unet", 3)]),
    "ddpm_tiled": (["ddpm_sample_tiled"], [3], [9], [False], [False], [4], [("tiled", 3, TILE)]),
    "ddpm_tiled_sched": (["ddpm_sample_tiled"], [3], [0], [False], [False], [0], [("tiled", 3, TILE)]),
    "ddpm_guided": (["ddpm_cfg_sample"], [3], [9], [True], [False], [4], [("ddpm_cfg", 3)]),
    "ddpm_guided_sched_sliced": (["ddpm_cfg_sample_sched"] * 2, [2, 1], [M64, 0], [True, True], [True, True], [0, 0], [("ddpm_cfg", 2), ("ddpm_cfg", 1)]),
    "ddpm_guided_injected_sliced": (["ddpm_cfg_sample"] * 3, [1, 1, 1], [9, 10, 11], [False] * 3, [True] * 3, [4, 4, 4], [("ddpm_cfg", 1)]),
    "ddpm_prediction_v": (["ddpm_pred_sample"], [3], [9], [False], [False], [0], [("ddpm_pred", 3, 0, 0)]),
    "multistep": (["ddpm_multistep_sample"], [3], [0], [False], [False], [None], [("ddpm_multistep", 3, 0)]),
    "multistep_unguided_is_not_sliced": (["ddpm_multistep_sample"], [3], [0], [False], [False], [None], [("ddpm_multistep", 3, 0)]),
    "multistep_guided_sliced": (["ddpm_multistep_cfg_sample"] * 2, [2, 1], [0, 0], [True, True], [True, True], [None, None],
                                [("ddpm_multistep", 2, 1), ("ddpm_multistep", 1, 1)]),
    "shaped": (["ddpm_shaped_sample"], [3], [9], [False], [False], [4], [("ddpm_shaped", 3, 0, 0)]),
    "shaped_unguided_is_one_call": (["ddpm_shaped_sample"], [3], [9], [False], [False], [0], [("ddpm_shaped", 3, 0, 0)]),
    "shaped_multistep_guided_sliced": (["ddpm_shaped_sample"] * 2, [2, 1], [9, 10], [True, True], [True, True], [0, 0],
                                       [("ddpm_shaped", 2, 1, 1), ("ddpm_shaped", 1, 1, 1)]),
    "learned": (["ddpm_lv_sample"], [3], [9], [False], [False], [4], [("ddpm_lv", 3, 0, 0)]),
    "learned_guided_sliced": (["ddpm_lv_sample"] * 2, [2, 1], [9, 10], [False, False], [True, True], [4, 4], [("ddpm_lv", 2, 1, 0), ("ddpm_lv", 1, 1, 0)]),
    "learned_multistep": (["ddpm_lv_sample"], [3], [0], [False], [False], [0], [("ddpm_lv", 3, 0, 1)]),
    "learned_times_only": (["ddpm_lv_sample"], [3], [9], [False], [False], [0], [("ddpm_lv", 3, 0, 0)]),
    "pred_x0": (["ddpm_pred_sample"], [3], [9], [False], [False], [4], [("ddpm_pred", 3, 0, 0)]),
    "pred_v_guided_shaped_sliced": (["ddpm_pred_sample"] * 2, [2, 1], [9, 10], [True, True], [True, True], [0, 0],
                                    [("ddpm_pred", 2, 1, 0), ("ddpm_pred", 1, 1, 0)]),
    "pred_x0_multistep": (["ddpm_pred_sample"], [3], [0], [False], [False], [0], [("ddpm_pred", 3, 0, 1)]),
    "vlb_fixed_injected": (["ddpm_vlb"], [3], [0], [False], [False], [4], [("ddpm_vlb", 3)]),
    "vlb_learned_philox": (["ddpm_vlb"], [3], [5], [True], [False], [0], [("ddpm_vlb", 3)]),
    "vlb_pred_x0": (["ddpm_vlb_pred"], [3], [0], [False], [False], [0], [("ddpm_vlb", 3)]),
    "vlb_philox_sliced": (["ddpm_vlb"] * 2, [2, 1], [M64, 0], [True, True], [False, False], [0, 0], [("ddpm_vlb", 2), ("ddpm_vlb", 1)]),
    "vlb_injected_sliced": (["ddpm_vlb_pred"] * 2, [2, 1], [0, 1], [False, False], [False, False], [4, 4], [("ddpm_vlb", 2), ("ddpm_vlb", 1)]),
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()   # tile plans come from the library's own host function


def observe(row):
    _, ekw, call = row
    eng = fake_engine(**ekw)
    call(eng, D())
    calls = eng.L.calls
    lo, rows_ok = 0, True
    for c in calls:   # consecutive calls of one sampler walk the batch: each gets its own rows
        if lo + c["B"] > B:
            lo = 0
        hi = lo + c["B"]
        rows_ok &= c["lab"] in (None, Y[lo:hi]) and c["wt"] in (None, WT[lo:hi])
        lo = hi % B
    return ([c["name"].replace("mi355_", "") for c in calls], [c["B"] for c in calls], [c["seed"] for c in calls],
            [c["lab"] is not None for c in calls], [c["wt"] is not None for c in calls], [c["nd"] for c in calls],
            [(s[0].replace("mi355_", "").replace("_workspace_bytes", ""),) + s[1:] for s in eng.L.sizes]), rows_ok


def test_every_row_is_expected_and_every_sampler_is_covered():
    from mi355.engine import UNetEngine

    assert sorted(EXPECT) == sorted(r[0] for r in ROWS)
    seen = {n for e in EXPECT.values() for n in e[0]}
    assert seen == {n.replace("mi355_", "") for n in POS}, "an entry point of POS that no row reaches"
    for m in ("forward", "forward_cached", "forward_tiled", "cfm_euler", "cfm_rk", "cfm_ab", "cfm_cfg", "cfm_recon", "sf2m_euler", "ddpm_sample",
              "ddpm_multistep", "ddpm_shaped", "ddpm_learned", "ddpm_pred", "ddpm_vlb"):
        assert callable(getattr(UNetEngine, m))


def test_ddpm_options_reach_the_library():
    """mi355_ddpm_options as the calls carry it: (mode, n_corrector, delta, tmin, tmax, start_fraction, noise_condition, pad_value, none_value,
    cond_is_none, seed).  The guided ddpm_sample path passes start_fraction 1, noise_condition 1, pad_value -2 whatever the caller gave."""
    L = _lib()
    eng, d = fake_engine(in_ch=2, max_batch=4), D()
    kw = dict(cond=d.x(), n_corrector=2, delta=0.25, tmin=0.125, tmax=0.5, start_fraction=0.5, noise_condition=False, pad_value=0.0, none_value=-1.0, seed=9)
    eng.ddpm_sample(d.x(), d.tables, mode=L.DDPM_AMORTIZED, **kw)
    eng.ddpm_sample(d.x(), d.tables, mode=L.DDPM_AMORTIZED, guidance_scale=2.0, **kw)
    eng.ddpm_shaped(d.x(), d.tables, None, mode=L.DDPM_AMORTIZED, guidance_scale=2.0, **kw)
    eng.ddpm_multistep(d.x(), d.tables, d.coefs, none_value=-1.0)
    eng.ddpm_sample(d.x(1), d.tables, mode=L.DDPM_PRIOR)
    m = L.DDPM_AMORTIZED
    assert [c["opt"] for c in eng.L.calls] == [
        (m, 2, 0.25, 0.125, 0.5, 0.5, 0, 0.0, -1.0, 0, 9),
        (m, 2, 0.25, 0.125, 0.5, 1.0, 1, -2.0, -1.0, 0, 9), (m, 2, 0.25, 0.125, 0.5, 1.0, 1, -2.0, -1.0, 0, 10),
        (m, 2, 0.25, 0.125, 0.5, 0.5, 0, 0.0, -1.0, 0, 9), (m, 2, 0.25, 0.125, 0.5, 0.5, 0, 0.0, -1.0, 0, 10),
        (L.DDIM, 0, C.c_float(0.1).value, C.c_float(1e-5).value, 1.0, 1.0, 1, -2.0, -1.0, 1, 0),
        (L.DDPM_PRIOR, 0, C.c_float(0.1).value, C.c_float(1e-5).value, 1.0, 1.0, 1, -2.0, -2.0, 1, 0)]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_dispatch(row):
    got, rows_ok = observe(row)
    want = EXPECT[row[0]]
    for what, g, w in zip(("entry points", "batch", "seed", "labels", "scales", "n_noise_draws", "workspace functions"), got, want):
        assert g == w, (row[0], what, g, w)
    assert rows_ok, "a slice did not receive its own rows of labels / per-image scales"
