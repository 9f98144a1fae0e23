"""Counterpart of `AD/image_diffusion/sampling.py`: the reverse-denoising samplers.

Same factories and call contracts as the reference:
    get_prior_sample_fn(eps_model, ddpm, conditioning, likelihood)        -> sample(xT)
    get_conditional_sample_fn(eps_model, ddpm, conditioning, likelihood)  -> sample(xT, condition)
`eps_model(xi, i)` takes a long [B] step-index tensor (experiments/main.py:140).  Dispatch is on
`type(conditioning)` (the reference uses the un-vendored `plum` package for that).

Two execution paths, both entirely on the HIP backend:
  * fast path - `eps_model` was made by `make_eps_model(network, ddpm)` with a `UNetModel`: the whole
    loop runs inside libmi355_sampler (`mi355_ddpm_sample`), one C call per sample() call;
  * generic path - any callable `eps_model` (e.g. the reference's own lambda around a UNetModel): a
    host loop that calls it once per step and applies the fused HIP step kernels (csrc/steps.hip).
Noise: by default drawn in-kernel (Philox4x32-10, seeded from torch.initial_seed()); parity tests
inject the draws of the reference's `torch.randn_like` call sequence with `injected_noise([...])`.
Build-defined extensions without a reference counterpart: get_ddim_sample_fn (DDIM(eta)) and get_dpm_solver_sample_fn (DPM-Solver++ multistep,
orders 1 and 2: one evaluation and one step kernel per step, the previous step's data prediction kept on the device).  A chain made by
DDPM.with_x0_shaping(...) has every sampler here end its predictor steps' data prediction per image (dynamic thresholding, guidance rescale) instead of
with the static clip: the fast path in mi355_ddpm_shaped_sample, the generic one through x0_shape_stats and x0_shaped_step_; sample quality untested.
A chain made by DDPM.with_learned_variance() samples a net with 2C outputs (eps | v, improved-DDPM's learned variance range): the fast path in
mi355_ddpm_lv_sample, the generic one through ddpm_lv_step_ and strided_step_ on the net's output as it is; DDPM.from_betas chains (linear, cosine;
a time_scale between step and network time) run there as well; sample quality untested.
A chain made by DDPM.with_prediction("x0" | "v") samples a net whose output is the data prediction or v: the fast path in mi355_ddpm_pred_sample,
the generic one through pred_step_ (and pred_shape_stats) on the net's raw output, one step op per step; make_eps_model keeps its name, the model
returns whatever the net writes; sample quality untested.
ReconstructionGuidance (sampling.py:136-206) differentiates the x0 model through the U-Net: the gradient is the HIP engine's
vector-Jacobian product (`UNetEngine.vjp`, csrc/unet_backward.hip) of a differentiable plan of the same network, so it needs an
`eps_model` made by `make_eps_model(network, ddpm)` around a `UNetModel`.
"""
from __future__ import annotations

import contextlib
import math
from typing import Callable, List, Optional

import torch

from mi355 import _lib
from mi355.ops import default_ops

from .conditioning import Amortized, ClassifierFreeGuidance, Conditioning, NullSpace, ReconstructionGuidance, RePaint, Replacement, repaint_walk
from .likelihoods import Likelihood
from .sde_diffusion import DDPM

_ops = default_ops
_injected: Optional[List[torch.Tensor]] = None
_draw_counter = 0   # device-noise draws (host loop) and fast-path calls so far: the fast path keys each call with it
_noise_offset = 0   # elements of the host-loop Philox stream consumed so far (always a multiple of 4)


@contextlib.contextmanager
def injected_noise(draws):
    """Use `draws` (list / stacked tensor of [B,C,H,W]) instead of device Philox, in reference call order."""
    global _injected
    prev = _injected
    _injected = list(draws)
    try:
        yield
    finally:
        _injected = prev


@contextlib.contextmanager
def use_ops(ops):
    """Swap the op table (tests pass a recording double to check the host logic without a GPU)."""
    global _ops
    prev = _ops
    _ops = ops
    try:
        yield
    finally:
        _ops = prev


def _sched_key(ddpm: DDPM):
    """What identifies a sampling schedule: the training step count, the kept steps (None: all of them) and, where it is not 1, the factor
    between a step's position and the time the net sees (DDPM.from_betas)."""
    key = (int(getattr(ddpm, "base_Ns", ddpm.Ns)), getattr(ddpm, "timesteps", None))
    ts = float(getattr(ddpm, "time_scale", 1.0))
    return key if ts == 1.0 else key + (ts,)


def make_eps_model(network, ddpm: DDPM):
    """eps_model(xi, i) = network(xi, 1.0*i/Ns) (loss_functions.py:18-19, experiments/main.py:140),
    tagged so the samplers can run the whole loop inside the C library.  On a RespacedDDPM step i sits at training index tau_i:
    eps_model(xi, i) = network(xi, tau_i / base_Ns), for an int i and for the long [B] tensor the samplers pass."""
    steps = getattr(ddpm, "timesteps", None)

    if steps is None and float(getattr(ddpm, "time_scale", 1.0)) == 1.0:
        def eps_model(xi, i):
            return network(xi, 1.0 * i / ddpm.Ns)
    else:
        # time(k) for every k, rounded on the host: a device tensor divided by a Python number is multiplied by its rounded reciprocal,
        # which need not be the correctly rounded quotient the fused loop feeds
        times = torch.tensor([ddpm.time(k) for k in range(ddpm.Ns)], dtype=torch.float32)

        def eps_model(xi, i):
            if isinstance(i, torch.Tensor):
                return network(xi, times.to(i.device)[i])
            return network(xi, ddpm.time(i))

    eps_model._mi355_network = network
    eps_model._mi355_Ns = ddpm.Ns
    eps_model._mi355_sched = _sched_key(ddpm)   # the fused loop evaluates the net at this schedule's times: only for this very schedule
    return eps_model


class _Noise:
    """Hands out one noise draw per reference `torch.randn_like` call.

    Device noise: every draw takes the next `stride` elements (this tensor's size rounded up to a multiple of 4, one Philox counter = 4
    elements) of the process-wide stream, starting where the previous draw - of this or of any earlier sampler call, whatever its batch
    size - ended.  `_noise_offset` counts elements consumed, so ranges never overlap; the first call of a process starts at 0."""

    def __init__(self, like: torch.Tensor):
        self.like = like
        self.injected = list(_injected) if _injected is not None else None
        self.seed = int(torch.initial_seed()) & ((1 << 63) - 1)
        self.k = 0
        n = like.numel()
        self.stride = (n + 3) // 4 * 4

    def next(self):
        """-> (z tensor or None, philox (seed, offset) or None)"""
        global _draw_counter, _noise_offset
        if self.injected is not None:
            if self.k >= len(self.injected):
                raise RuntimeError("injected noise exhausted")
            z = self.injected[self.k].to(self.like.device, torch.float32).contiguous()
            self.k += 1
            return z, None
        off = _noise_offset
        _noise_offset += self.stride
        self.k += 1
        _draw_counter += 1
        return None, (self.seed, off)


def process_x0(img):
    return _ops.clip_(img, -1.0, 1.0)


def _same_schedule(eps_model, ddpm: DDPM) -> bool:
    """eps_model was built for ddpm's step count and its very schedule (a model tagged with a step count alone: the unrespaced chain of it)."""
    Ns = getattr(eps_model, "_mi355_Ns", None)
    return Ns == ddpm.Ns and getattr(eps_model, "_mi355_sched", (Ns, None)) == _sched_key(ddpm)


def _fast_engine(eps_model, ddpm: DDPM, xT: torch.Tensor):
    net = getattr(eps_model, "_mi355_network", None)
    if net is None or not _same_schedule(eps_model, ddpm) or not hasattr(net, "engine") or not xT.is_cuda:
        return None
    return net.engine(xT.device)


def _none_value(likelihood: Likelihood, like: torch.Tensor) -> float:
    return float(likelihood.pad_value) if hasattr(likelihood, "pad_value") else 0.0


def _tables(ddpm: DDPM):
    return ddpm.host_tables()


def _shaping_of(ddpm, guided: bool):
    """ddpm.x0_shaping (DDPM.with_x0_shaping; None on a plain chain), refused where it asks an unguided sampler for the guidance rescale."""
    shaping = getattr(ddpm, "x0_shaping", None)
    if shaping is not None and shaping.guidance_rescale > 0.0 and not guided:
        raise ValueError("guidance_rescale > 0 rescales the guided eps against the conditional one: it needs a guided sampler "
                         "(ClassifierFreeGuidance, or guidance_scale=)")
    return shaping


def _pred_of(ddpm, *, tiling=None, feature_cache=None) -> str:
    """ddpm.prediction (DDPM.with_prediction; "eps" on a plain chain); refused, by name, with what is not built for an x0- or v-prediction
    chain, and with a fixed large variance on a learned-variance chain (which of the two variances is meant?)."""
    pred = getattr(ddpm, "prediction", "eps")
    if getattr(ddpm, "fixed_variance", "small") == "large" and getattr(ddpm, "learned_variance", False):
        raise NotImplementedError('a fixed variance (DDPM.with_fixed_variance("large")) is not built for a learned-variance chain '
                                  "(DDPM.with_learned_variance): the chain has one variance")
    if pred == "eps":
        return pred
    if tiling is not None:
        raise NotImplementedError("tiling is not built for an x0- or v-prediction chain (DDPM.with_prediction)")
    if feature_cache is not None:
        raise NotImplementedError("feature_cache is not built for an x0- or v-prediction chain (DDPM.with_prediction)")
    return pred


def _pred_kw(T, i):
    """sa, sb of step i for pred_step_ / pred_shape_stats (read by the "v" kind)."""
    return dict(sa=float(T["sqrt_alphas_cumprod"][i]), sb=float(T["sqrt_one_minus_alphas_cumprod"][i]))


def _shape_rows(xi, eps, i, T, shaping, w=None, pred="eps"):
    """The per-image rows (f, s) of step i's shaped data prediction, or None without shaping.  w: eps is the [2B] pair of a guided step.
    pred (not "eps"): eps is the raw output of an x0- or v-prediction net."""
    if shaping is None:
        return None
    if pred != "eps":
        return _ops.pred_shape_stats(pred, xi, eps, float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i]), shaping, w=w,
                                     **_pred_kw(T, i))
    return _ops.x0_shape_stats(xi, eps, float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i]), shaping, w=w)


def _learned_of(ddpm, *, tiling=None, feature_cache=None):
    """ddpm.max_log() of a learned-variance chain (DDPM.with_learned_variance), None on a plain one; refused, by name, with what is not built
    for such a chain."""
    if not getattr(ddpm, "learned_variance", False):
        return None
    if getattr(ddpm, "x0_shaping", None) is not None:
        raise NotImplementedError("per-image x0_shaping (DDPM.with_x0_shaping) is not built for a learned-variance chain (DDPM.with_learned_variance)")
    if tiling is not None:
        raise NotImplementedError("tiling is not built for a learned-variance chain (DDPM.with_learned_variance)")
    if feature_cache is not None:
        raise NotImplementedError("feature_cache is not built for a learned-variance chain (DDPM.with_learned_variance)")
    return ddpm.max_log()


def _check_width(out_channels, xi, max_log, host_loop=False):
    """The channels the net writes against the chain: the state's C, or 2C (eps | v) on a learned-variance chain.  host_loop: a plain chain is
    left to the step ops, which refuse an eps that has not the state's shape."""
    if host_loop and max_log is None:
        return
    if out_channels != xi.shape[1] * (2 if max_log is not None else 1):
        raise ValueError(f"the net writes {out_channels} channels for a state of {xi.shape[1]}: " +
                         ("a learned-variance chain (DDPM.with_learned_variance) needs a net with twice the state's channels (eps | v)"
                          if max_log is not None else "a net with twice the state's channels (learn_sigma) needs ddpm.with_learned_variance()"))


def _check_engine_width(engine, xi, max_log):
    """_check_width of a fused call: the engine's net against the chain, where learned variance is in play (a learned chain, or a 2C-output
    net on a plain one); any other width is the library's own refusal."""
    out_channels = getattr(engine, "out_channels", None)
    if out_channels is not None and (max_log is not None or out_channels == 2 * xi.shape[1]):
        _check_width(out_channels, xi, max_log)


def _predictor(eps, xi, i, T, noise: _Noise, shape=None, max_log=None, w=None, pred="eps"):
    """step() (sampling.py:59-67): x0_hat -> clip -> posterior mean -> + exp(0.5 logvar) z (z iff i > 0).  shape: the rows of _shape_rows
    (per-image shaping in place of the clip).  max_log (a learned-variance chain): eps is the net's 2C output, passed whole; with w, the
    [2B] pair of a guided step and xi the duplicated state.  pred (not "eps"): eps is the raw output of an x0- or v-prediction net, passed
    whole to the one step op that takes the kind."""
    z, ph = noise.next() if i > 0 else (None, None)
    sigma = float((0.5 * T["posterior_log_variance_clipped"][i]).exp())  # fp32, like (0.5*logvar).exp()
    if pred != "eps":
        cr, crm1 = float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i])
        c1, c2 = float(T["posterior_mean_coef1"][i]), float(T["posterior_mean_coef2"][i])
        if max_log is not None and i > 0:
            return _ops.pred_step_("ddpm_lv", pred, xi, eps, cr, crm1, c1, c2, min_log=float(T["posterior_log_variance_clipped"][i]),
                                   max_log=float(max_log[i]), z=z, philox=ph, w=w, **_pred_kw(T, i))
        return _ops.pred_step_("ddpm", pred, xi, eps, cr, crm1, c1, c2, sigma=sigma, z=z, philox=ph, w=w, shape=shape, **_pred_kw(T, i))
    if max_log is not None:
        cr, crm1 = float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i])
        c1, c2 = float(T["posterior_mean_coef1"][i]), float(T["posterior_mean_coef2"][i])
        if i > 0:
            return _ops.ddpm_lv_step_(xi, eps, z, cr, crm1, c1, c2, float(T["posterior_log_variance_clipped"][i]), float(max_log[i]), ph, w=w)
        return _ops.strided_step_("ddpm", xi, eps, cr, crm1, c1, c2, sigma=sigma, w=w)   # step 0 draws no noise and never reads v
    if shape is not None:
        _ops.x0_shaped_step_("ddpm", xi, eps, shape, float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i]),
                             float(T["posterior_mean_coef1"][i]), float(T["posterior_mean_coef2"][i]), sigma=sigma, z=z, philox=ph)
        return xi
    _ops.ddpm_step_(xi, eps, z, float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i]),
                    float(T["posterior_mean_coef1"][i]), float(T["posterior_mean_coef2"][i]), sigma, ph)
    return xi


def _corrector(eps, xi, i, T, ddpm, delta, noise: _Noise, max_log=None, pred="eps"):
    """corrector_step (sampling.py:113-121).  max_log (a learned-variance chain): eps is the net's 2C output, passed whole.  pred: as in
    _predictor."""
    z, ph = noise.next()
    dt = (ddpm.tmax - ddpm.tmin) / ddpm.Ns
    if pred != "eps":
        return _ops.pred_step_("corrector", pred, xi, eps, float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i]),
                               float(T["recip_sqrt_m1_alphas_cumprod"][i]), dt, float(delta), z=z, philox=ph, **_pred_kw(T, i))
    if max_log is not None:
        return _ops.strided_step_("corrector", xi, eps, float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i]),
                                  float(T["recip_sqrt_m1_alphas_cumprod"][i]), dt, float(delta), z=z, philox=ph)
    _ops.corrector_step_(xi, eps, z, float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i]),
                         float(T["recip_sqrt_m1_alphas_cumprod"][i]), dt, float(delta), ph)
    return xi


def _times(xi, i):
    return torch.full((xi.shape[0],), i, device=xi.device, dtype=torch.long)


def _net_in(xi, cond, amortized):
    return torch.concat((xi, cond), dim=-3) if amortized else xi  # sampling.py:39 (plumbing: the net's own input)


def _walk_moves(Ns, walk):
    """(level, down) per move of a walk over the levels Ns..0 (None: the plain descent); down: step level - 1 runs, else the level re-noises."""
    if walk is None:
        return [(L, True) for L in range(Ns, 0, -1)]
    if len(walk) < 1 or walk[0] != Ns or walk[-1] != 0 or any(abs(b - a) != 1 or not 0 <= b <= Ns for a, b in zip(walk, walk[1:])):
        raise ValueError("walk must start at level Ns, end at level 0 and move by +-1")
    return [(a, b < a) for a, b in zip(walk, walk[1:])]


def _run_generic(eps_model, ddpm, xT, *, amortized, cond_pred, cond_corr, replacement=None, n_corrector=0, delta=0.1, walk=None):
    T = _tables(ddpm)
    shaping = _shaping_of(ddpm, False)
    max_log = _learned_of(ddpm)
    pred = _pred_of(ddpm)
    xi = xT.detach().clone().float().contiguous()
    noise = _Noise(xi)
    for level, down in _walk_moves(ddpm.Ns, walk):
        if not down:   # q(x_level+1 | x_level): one draw
            z, ph = noise.next()
            _ops.renoise_(xi, z, float(T["alphas"][level].sqrt()), float(T["betas"][level].sqrt()), ph)
            continue
        i = level - 1
        if replacement is not None and i < int(ddpm.Ns * replacement["start_fraction"]):
            z, ph = noise.next() if replacement["noise"] else (None, None)
            _ops.replace_mask_(xi, replacement["condition"], z, replacement["pad_value"], replacement["noise"],
                               float(T["sqrt_alphas_cumprod"][i]), float(T["sqrt_one_minus_alphas_cumprod"][i]), ph)
        eps = eps_model(_net_in(xi, cond_pred, amortized), _times(xi, i)).float().contiguous()
        _check_width(eps.shape[1], xi, max_log, host_loop=True)
        _predictor(eps, xi, i, T, noise, _shape_rows(xi, eps, i, T, shaping, pred=pred), max_log, pred=pred)
        for _ in range(n_corrector):
            eps = eps_model(_net_in(xi, cond_corr, amortized), _times(xi, i))
            _corrector(eps.float().contiguous(), xi, i, T, ddpm, delta, noise, max_log, pred=pred)
    return process_x0(xi)


def _ddim_move(eps, xi, i, T, sigma, noise, shape=None, wide=False, w=None, pred="eps"):
    """One DDIM step: sigma None = the deterministic kernel; else DDIM(eta) with sigma[i] and one draw iff i > 0.  shape: as in _predictor.
    wide (a learned-variance chain): eps is the net's 2C output, passed whole; with w, the [2B] pair of a guided step, xi the duplicated state."""
    cr, crm1, prev = float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i]), float(T["alphas_cumprod_prev"][i])
    if pred != "eps":   # the raw output of an x0- or v-prediction net, passed whole (wide or not) to the one step op that takes the kind
        if sigma is None:
            return _ops.pred_step_("ddim", pred, xi, eps, cr, crm1, prev, w=w, shape=shape, **_pred_kw(T, i))
        z, ph = noise.next() if i > 0 else (None, None)
        return _ops.pred_step_("ddim_eta", pred, xi, eps, cr, crm1, prev, sigma=float(sigma[i]), z=z, philox=ph, w=w, shape=shape, **_pred_kw(T, i))
    if wide:
        if sigma is None:
            return _ops.strided_step_("ddim", xi, eps, cr, crm1, prev, w=w)
        z, ph = noise.next() if i > 0 else (None, None)
        return _ops.strided_step_("ddim_eta", xi, eps, cr, crm1, prev, sigma=float(sigma[i]), z=z, philox=ph, w=w)
    if sigma is None:
        return _ops.ddim_step_(xi, eps, cr, crm1, prev) if shape is None else _ops.x0_shaped_step_("ddim", xi, eps, shape, cr, crm1, prev)
    z, ph = noise.next() if i > 0 else (None, None)
    if shape is not None:
        return _ops.x0_shaped_step_("ddim_eta", xi, eps, shape, cr, crm1, prev, sigma=float(sigma[i]), z=z, philox=ph)
    return _ops.ddim_eta_step_(xi, eps, z, cr, crm1, prev, float(sigma[i]), ph)


def _run_generic_cfg(eps_model, ddpm, xT, *, cond, none, guidance_scale, n_corrector=0, delta=0.1, ddim=False, ddim_sigma=None):
    """The guided host loop for any eps_model callable: two calls per predictor step (condition, none_like), cfg_combine, the step kernel;
    correctors as in _run_generic (the net sees none_like).  With shaping the rows come from the pair (the rescale needs eps_c beside eps_g)."""
    T = _tables(ddpm)
    shaping = _shaping_of(ddpm, True)
    max_log = _learned_of(ddpm)
    pred = _pred_of(ddpm)
    xi = xT.detach().clone().float().contiguous()
    noise = _Noise(xi)
    B = xi.shape[0]
    for i in reversed(range(ddpm.Ns)):
        ec = eps_model(_net_in(xi, cond, True), _times(xi, i)).float()
        eu = eps_model(_net_in(xi, none, True), _times(xi, i)).float()
        eps2 = torch.cat((ec, eu)).contiguous()
        _check_width(eps2.shape[1], xi, max_log, host_loop=True)
        if max_log is not None or pred != "eps":
            # the guided step kernels on the pair itself (a 2C pair: v from the conditional half; an x0- or v-prediction pair: mixed raw), the
            # state duplicated for them
            x2 = torch.cat((xi, xi))
            shape = _shape_rows(xi, eps2, i, T, shaping, w=guidance_scale, pred=pred) if pred != "eps" else None
            if ddim:
                _ddim_move(eps2, x2, i, T, ddim_sigma, noise, shape, wide=True, w=guidance_scale, pred=pred)
            else:
                _predictor(eps2, x2, i, T, noise, shape, max_log=max_log, w=guidance_scale, pred=pred)
            xi.copy_(x2[:B])
            for _ in range(0 if ddim else n_corrector):
                eps = eps_model(_net_in(xi, none, True), _times(xi, i))
                _corrector(eps.float().contiguous(), xi, i, T, ddpm, delta, noise, max_log, pred=pred)
            continue
        shape = _shape_rows(xi, eps2, i, T, shaping, w=guidance_scale)
        eps = _ops.cfg_combine(eps2, guidance_scale)
        if ddim:
            _ddim_move(eps, xi, i, T, ddim_sigma, noise, shape)
            continue
        _predictor(eps, xi, i, T, noise, shape)
        for _ in range(n_corrector):
            eps = eps_model(_net_in(xi, none, True), _times(xi, i))
            _corrector(eps.float().contiguous(), xi, i, T, ddpm, delta, noise)
    return process_x0(xi)


class FeatureCache:
    """Feature reuse across the network evaluations of a sampler (DeepCache: Ma, Fang, Wang, CVPR 2024; training-free; BUILD-DEFINED
    EXTENSION, no reference counterpart): the deep features of the U-Net are recomputed on a schedule and reused in between, only the
    `branch` outermost block pairs run at every evaluation.  interval=N: one full evaluation in N (full at evaluation e iff e % N == 0);
    schedule: the explicit list, one truth value per evaluation in loop order (correctors included; the first must be true); branch: 1..n-1,
    see UNetEngine.cache_branches() for what each branch keeps and costs.  Taken by the sample functions that end in UNetEngine.ddpm_sample
    (prior, amortized, replacement / RePaint, DDIM, on respaced chains too): as feature_cache= of get_prior_sample_fn and
    get_conditional_sample_fn, or carried by the chain, ddpm.with_feature_cache(FeatureCache(...)), which get_ddim_sample_fn reads as well;
    the guided, reconstruction-guided, multistep and shaped loops refuse it.  Sample quality under feature reuse is untested (no trained checkpoint is at hand); the arithmetic
    is tested against an fp64 / fp32 restatement."""

    def __init__(self, interval=None, schedule=None, branch=1):
        if (interval is None) == (schedule is None):
            raise ValueError("FeatureCache needs exactly one of interval= and schedule=")
        self.interval, self.schedule, self.branch = interval, (None if schedule is None else tuple(bool(f) for f in schedule)), int(branch)

    def kwargs(self):
        return dict(cache_interval=self.interval, cache_schedule=self.schedule, cache_branch=self.branch)


class Tiling:
    """Tiled sampling of canvases larger than the network's frame (MultiDiffusion: Bar-Tal et al., ICML 2023; training-free; BUILD-DEFINED
    EXTENSION, no reference counterpart): at every network evaluation the canvas [B, C, Hc, Wc] (Hc, Wc >= image_size) is cut into overlapping
    image_size windows, the net runs on all windows as a batch, and the predictions are fused per pixel by a weighted average; the sampler's own
    step is then taken on the canvas.  stride: an int or (sy, sx) in 1..image_size (None: image_size // 2); weight: "uniform" (the plain
    average) or "tent" (fades the seams); chunk: windows per forward (None: all of a call's, up to the engine's max_batch()).  Taken as tiling=
    by get_prior_sample_fn and get_conditional_sample_fn (Amortized, Replacement, RePaint), or carried by the chain,
    ddpm.with_tiling(Tiling(...)), which get_ddim_sample_fn reads as well (the fused path only); and by torchcfm_compat.NeuralODE.  The guided,
    reconstruction-guided, multistep, shaped and cached loops refuse it.  Sample quality under tiling is
    untested (no trained checkpoint is at hand); the arithmetic is tested against an fp64 / fp32 restatement."""

    def __init__(self, stride=None, weight="uniform", chunk=None):
        if weight not in _lib.TILE_WEIGHTS:
            raise ValueError(f"Tiling weight must be one of {sorted(_lib.TILE_WEIGHTS)}, got {weight!r}")
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f"Tiling chunk must be >= 1, got {chunk}")
        self.stride, self.weight, self.chunk = stride, weight, (None if chunk is None else int(chunk))


def _tiling_of(ddpm, tiling=None):
    """The tiling a sample function runs under: its own argument, else the chain's (DDPM.with_tiling)."""
    return tiling if tiling is not None else getattr(ddpm, "tiling", None)


def _refuse_tiling(tiling, loop: str):
    if tiling is not None:
        raise NotImplementedError(f"tiling is not built for {loop} (it runs with the prior, amortized, replacement / RePaint and DDIM samplers)")


def _need_fused_tiling(engine, tiling):
    if tiling is not None and engine is None:
        raise NotImplementedError("tiling runs inside the fused loop: pass an eps_model built by make_eps_model(network, ddpm) for this "
                                  "schedule and device tensors (an arbitrary callable sees whole frames only)")


def _cache_of(ddpm, feature_cache=None):
    """The cache a sample function runs under: its own argument, else the chain's (DDPM.with_feature_cache)."""
    return feature_cache if feature_cache is not None else getattr(ddpm, "feature_cache", None)


def _refuse_feature_cache(feature_cache, loop: str):
    if feature_cache is not None:
        raise NotImplementedError(f"feature_cache is not built for {loop} (it runs with the prior, amortized, replacement / RePaint and DDIM samplers)")


def _run_fast(engine, ddpm, xT, mode, cond, *, n_corrector=0, delta=0.1, start_fraction=1.0, noise_condition=True,
              pad_value=-2.0, none_value=-2.0, guidance_scale=None, ddim_sigma=None, walk=None, feature_cache=None, tiling=None):
    global _draw_counter
    xi = xT.detach().clone().float().contiguous()
    noise = None
    seed = int(torch.initial_seed()) & ((1 << 63) - 1)
    if _injected is not None:
        noise = torch.stack([z.to(xi.device, torch.float32) for z in _injected]).contiguous()
    else:
        seed = (seed + 0x9E3779B97F4A7C15 * (_draw_counter + 1)) & ((1 << 63) - 1)
        _draw_counter += 1
    sched = {}
    if getattr(ddpm, "timesteps", None) is not None or ddim_sigma is not None or walk is not None:
        # the scheduled entry points: a respaced chain's steps in training time (an unrespaced one's: 0..Ns-1 of Ns)
        sched = dict(timesteps=getattr(ddpm, "timesteps", None) or tuple(range(ddpm.Ns)), train_steps=int(getattr(ddpm, "base_Ns", ddpm.Ns)),
                     ddim_sigma=ddim_sigma, walk=walk)
    kw = dict(mode=mode, cond=cond, noise=noise, n_corrector=n_corrector, delta=float(delta), tmin=ddpm.tmin, tmax=ddpm.tmax,
              start_fraction=float(start_fraction), noise_condition=bool(noise_condition), pad_value=float(pad_value), none_value=float(none_value),
              seed=seed, guidance_scale=guidance_scale, **sched)
    shaping = _shaping_of(ddpm, guidance_scale is not None)
    feature_cache = _cache_of(ddpm, feature_cache)
    tiling = _tiling_of(ddpm, tiling)
    max_log = _learned_of(ddpm, tiling=tiling, feature_cache=feature_cache)
    pred = _pred_of(ddpm, tiling=tiling, feature_cache=feature_cache)
    times = _custom_times(ddpm)
    _check_engine_width(engine, xi, max_log)
    if pred != "eps":   # an x0- or v-prediction net: mi355_ddpm_pred_sample, which takes the shaping, the variance range and the times beside the kind
        engine.ddpm_pred(xi, _tables(ddpm), pred, shaping=shaping, max_log=max_log, times=times, **kw)
        return xi
    if feature_cache is not None:
        if guidance_scale is not None:
            _refuse_feature_cache(feature_cache, "the guided (classifier-free guidance) loops")
        if shaping is not None:
            _refuse_feature_cache(feature_cache, "the shaped loops (DDPM.with_x0_shaping)")
        kw.update(feature_cache.kwargs())
    if tiling is not None:
        if guidance_scale is not None:
            _refuse_tiling(tiling, "the guided (classifier-free guidance) loops")
        if shaping is not None:
            _refuse_tiling(tiling, "the shaped loops (DDPM.with_x0_shaping)")
        if feature_cache is not None:
            raise NotImplementedError("tiling together with feature_cache is not built")
        kw["tiling"] = tiling
    if max_log is not None or times is not None:   # a learned variance range and / or the chain's own times: mi355_ddpm_lv_sample
        for what, v in (("x0_shaping", shaping), ("tiling", tiling), ("feature_cache", feature_cache)):
            if v is not None:
                raise NotImplementedError(f"{what} is not built for a chain with a time_scale (DDPM.from_betas(..., time_scale=))")
        engine.ddpm_learned(xi, _tables(ddpm), max_log, times=times, **kw)
    elif shaping is not None:   # the same loop with per-image shaping of x0_hat: mi355_ddpm_shaped_sample
        engine.ddpm_shaped(xi, _tables(ddpm), shaping, **kw)
    else:
        engine.ddpm_sample(xi, _tables(ddpm), **kw)
    return xi


def _custom_times(ddpm):
    """The K times the net sees on a chain whose time_scale is not 1 (DDPM.from_betas), None where the fused loops' own rule holds."""
    if float(getattr(ddpm, "time_scale", 1.0)) == 1.0:
        return None
    return torch.tensor([ddpm.time(k) for k in range(ddpm.Ns)], dtype=torch.float32)


# Prior sampling ------------------------------------------------------------------------------------

def _need_fused(engine, feature_cache):
    if feature_cache is not None and engine is None:
        raise NotImplementedError("feature_cache runs inside the fused loop: pass an eps_model built by make_eps_model(network, ddpm) for this "
                                  "schedule and device tensors (an arbitrary callable is evaluated whole)")


def get_prior_sample_fn(eps_model: Callable, ddpm: DDPM, conditioning: Conditioning, likelihood: Likelihood, feature_cache=None, tiling=None):
    """sampling.py:50-75.  Under Amortized conditioning the net is fed `likelihood.none_like` (sampling.py:36-37).
    feature_cache (None: untouched): a FeatureCache.  tiling (None: the chain's, ddpm.tiling; neither: untouched): a Tiling; xT is then a canvas."""
    amortized = isinstance(conditioning, Amortized)
    feature_cache = _cache_of(ddpm, feature_cache)
    tiling = _tiling_of(ddpm, tiling)
    _learned_of(ddpm, tiling=tiling, feature_cache=feature_cache)   # a learned-variance chain: its refusals, before the first sample
    _pred_of(ddpm, tiling=tiling, feature_cache=feature_cache)      # an x0- or v-prediction chain: likewise

    @torch.no_grad()
    def sample(xT):
        engine = _fast_engine(eps_model, ddpm, xT)
        _need_fused(engine, feature_cache)
        _need_fused_tiling(engine, tiling)
        if engine is not None:
            return _run_fast(engine, ddpm, xT, _lib.DDPM_PRIOR, None, none_value=_none_value(likelihood, xT), feature_cache=feature_cache,
                             tiling=tiling)
        none = likelihood.none_like(xT) if amortized else None
        return _run_generic(eps_model, ddpm, xT, amortized=amortized, cond_pred=none, cond_corr=none)

    return sample


# Conditional sampling ---------------------------------------------------------------------------------

def get_conditional_sample_fn(eps_model: Callable, ddpm: DDPM, conditioning: Conditioning, likelihood: Likelihood, feature_cache=None, tiling=None):
    """feature_cache (None: the chain's, ddpm.feature_cache; neither: untouched): a FeatureCache; Amortized, Replacement and RePaint take it, the
    other conditionings refuse it by name.  tiling (None: the chain's, ddpm.tiling; neither: untouched): a Tiling, xT and the condition are then
    canvases; taken and refused by the same conditionings."""
    feature_cache = _cache_of(ddpm, feature_cache)
    tiling = _tiling_of(ddpm, tiling)
    _learned_of(ddpm, tiling=tiling, feature_cache=feature_cache)   # a learned-variance chain: its refusals, before the first sample
    _pred_of(ddpm, tiling=tiling, feature_cache=feature_cache)      # an x0- or v-prediction chain: likewise
    if isinstance(conditioning, ClassifierFreeGuidance):   # (an Amortized: before it)
        _refuse_feature_cache(feature_cache, "ClassifierFreeGuidance (the guided loops)")
        _refuse_tiling(tiling, "ClassifierFreeGuidance (the guided loops)")
        return _cfg_sample_fn(eps_model, ddpm, conditioning, likelihood)
    if isinstance(conditioning, Amortized):
        return _amortized_sample_fn(eps_model, ddpm, conditioning, likelihood, feature_cache, tiling)
    if isinstance(conditioning, RePaint):   # (a Replacement: before it)
        return _replacement_sample_fn(eps_model, ddpm, conditioning, likelihood, walk=repaint_walk(ddpm.Ns, conditioning.jump_length,
                                                                                                   conditioning.n_resample), feature_cache=feature_cache,
                                      tiling=tiling)
    if isinstance(conditioning, Replacement):
        return _replacement_sample_fn(eps_model, ddpm, conditioning, likelihood, feature_cache=feature_cache, tiling=tiling)
    if isinstance(conditioning, NullSpace):
        _refuse_feature_cache(feature_cache, "NullSpace (the null-space loop)")
        _refuse_tiling(tiling, "NullSpace (the null-space loop)")
        return _nullspace_sample_fn(eps_model, ddpm, conditioning, likelihood)
    if isinstance(conditioning, ReconstructionGuidance):
        _refuse_feature_cache(feature_cache, "ReconstructionGuidance (the backward pass needs a whole forward)")
        _refuse_tiling(tiling, "ReconstructionGuidance (the backward pass needs a whole forward)")
        return _reconstruction_guidance_sample_fn(eps_model, ddpm, conditioning, likelihood)
    raise NotImplementedError(f"no sampler for conditioning type {type(conditioning).__name__}")


def _amortized_sample_fn(eps_model, ddpm, conditioning: Amortized, likelihood, feature_cache=None, tiling=None):
    """sampling.py:80-133.  The corrector calls the x0 model WITHOUT the condition (sampling.py:116), so the
    network sees none_like there - reproduced."""

    @torch.no_grad()
    def sample(xT, condition):
        condition = condition.to(xT.device).float().contiguous()
        engine = _fast_engine(eps_model, ddpm, xT)
        _need_fused(engine, feature_cache)
        _need_fused_tiling(engine, tiling)
        if engine is not None:
            return _run_fast(engine, ddpm, xT, _lib.DDPM_AMORTIZED, condition, n_corrector=conditioning.n_corrector,
                             delta=conditioning.delta, none_value=_none_value(likelihood, xT), feature_cache=feature_cache, tiling=tiling)
        return _run_generic(eps_model, ddpm, xT, amortized=True, cond_pred=condition, cond_corr=likelihood.none_like(xT),
                            n_corrector=conditioning.n_corrector, delta=conditioning.delta)

    return sample


def _cfg_sample_fn(eps_model, ddpm, conditioning: ClassifierFreeGuidance, likelihood):
    """Amortized sampling with the predictor's eps guided: eps_u + guidance_scale * (eps_c - eps_u), eps_u from likelihood.none_like.
    Fast path: the whole loop in mi355_ddpm_cfg_sample (one forward at twice the batch per predictor step); generic path: two eps_model
    calls per predictor step and the cfg_combine kernel.  The corrector is the amortized sampler's."""

    @torch.no_grad()
    def sample(xT, condition):
        condition = condition.to(xT.device).float().contiguous()
        w = float(conditioning.guidance_scale)
        engine = _fast_engine(eps_model, ddpm, xT)
        if engine is not None:
            return _run_fast(engine, ddpm, xT, _lib.DDPM_AMORTIZED, condition, n_corrector=conditioning.n_corrector,
                             delta=conditioning.delta, none_value=_none_value(likelihood, xT), guidance_scale=w)
        return _run_generic_cfg(eps_model, ddpm, xT, cond=condition, none=likelihood.none_like(xT), guidance_scale=w,
                                n_corrector=conditioning.n_corrector, delta=conditioning.delta)

    return sample


def _reconstruction_guidance_sample_fn(eps_model, ddpm, conditioning: ReconstructionGuidance, likelihood):
    """sampling.py:136-206.  Per step i < int(Ns * start_fraction):
        x_grad = vmap(grad(lambda xi: likelihood.loss(x0_model(xi, i), y)))(xi)      (x0_model = clip(predict_start_from_noise(eps_model)))
        x_update = -gamma * alpha_i * (1 - alpha_i) * x_grad;  "before": xi += x_update (the predictor then runs on the moved xi),
        "after": the predictor runs on xi and x_update is added to its result.
    The losses are per sample and the network has no cross-sample coupling, so vmap(grad) is ONE batched backward pass:
    seed kernel (clip / loss / predict_start chain rule) -> UNetEngine.vjp -> update kernel.  The guided steps' forward and VJP run on the
    differentiable plan, which is bf16 when the model's precision is 'fp16' (use_fp16=True) or 'bf16x2' (the backward exists in fp32 and bf16
    only, UNetModel.engine); the unguided steps and correctors keep the model's precision."""
    net = getattr(eps_model, "_mi355_network", None)
    if net is None or not _same_schedule(eps_model, ddpm) or not hasattr(net, "engine"):
        raise NotImplementedError(
            "ReconstructionGuidance differentiates through the network: pass an eps_model built by make_eps_model(network, ddpm) around "
            "a UNetModel (an arbitrary callable has no backward pass on the HIP backend)")
    if conditioning.update_rule not in ("before", "after"):
        raise ValueError(f"unknown update_rule {conditioning.update_rule!r}")
    if getattr(ddpm, "prediction", "eps") != "eps":
        raise NotImplementedError("ReconstructionGuidance is not built for an x0- or v-prediction chain (DDPM.with_prediction): the seed "
                                  "differentiates x0_hat = c_recip x - c_recipm1 eps of an eps net")
    if getattr(ddpm, "learned_variance", False):
        raise NotImplementedError("ReconstructionGuidance is not built for a learned-variance chain (DDPM.with_learned_variance): the seed and "
                                  "the backward pass take a net that writes the state's channels")
    if getattr(ddpm, "x0_shaping", None) is not None:
        raise NotImplementedError("ReconstructionGuidance differentiates the clipped x0_hat through the network: per-image x0 shaping "
                                  "(DDPM.with_x0_shaping) is not built into that gradient - pass the unshaped chain")
    if hasattr(likelihood, "pad_value"):
        mode, pad = 0, float(likelihood.pad_value)      # Painting.loss (likelihoods.py:58-66)
    elif type(likelihood).__name__ == "HyperResolution":
        mode, pad = 1, 0.0                              # HyperResolution.loss (likelihoods.py:138-143)
    elif type(likelihood).__name__ == "LowResolution":
        mode, pad = 2, 0.0                              # mean((D(x0) - y)^2), D the bilinear reduction: mi355_lowres_seed
    else:
        raise NotImplementedError(f"no constraint gradient for likelihood {type(likelihood).__name__}")

    @torch.no_grad()
    def sample(xT, condition):
        if not xT.is_cuda:
            from mi355._lib import MI355BackendError
            raise MI355BackendError("ReconstructionGuidance sampling needs device tensors (no CPU fallback)")
        T = _tables(ddpm)
        alphas = ddpm.alphas.detach().to("cpu", torch.float32)
        condition = condition.to(xT.device).float().contiguous()
        xi = xT.detach().clone().float().contiguous()
        B = xi.shape[0]
        deng, eng = net.engine(xi.device, differentiable=True), net.engine(xi.device)
        noise = _Noise(xi)
        n_guided = int(ddpm.Ns * conditioning.start_fraction)
        for i in reversed(range(ddpm.Ns)):
            t = torch.full((B,), ddpm.time(i), device=xi.device, dtype=torch.float32)
            update, eps = None, None
            if i < n_guided:
                eps = deng.forward(xi, t)
                if mode == 2:
                    g_eps, g_x, _ = _ops.lowres_seed(xi, eps, condition, float(T["sqrt_recip_alphas_cumprod"][i]),
                                                     float(T["sqrt_recipm1_alphas_cumprod"][i]))
                else:
                    g_eps, g_x = _ops.guidance_seed(xi, eps, condition, float(T["sqrt_recip_alphas_cumprod"][i]),
                                                    float(T["sqrt_recipm1_alphas_cumprod"][i]), mode, pad)
                vjp = deng.vjp(g_eps)
                a_i = float(alphas[i])
                scale = float(conditioning.gamma) * a_i * (1.0 - a_i)
                before = conditioning.update_rule == "before"
                update = _ops.guidance_update_(xi, g_x, vjp, scale, before)
                if before:
                    eps = None                       # xi moved: the predictor needs the network at the new point
            if eps is None:
                eps = eng.forward(xi, t)
            _predictor(eps, xi, i, T, noise)
            if update is not None and conditioning.update_rule == "after":
                _ops.euler_step_(xi, update, 1.0)    # pred_img += x_update
            for _ in range(conditioning.n_corrector):
                epc = eng.forward(xi, t)
                _corrector(epc, xi, i, T, ddpm, conditioning.delta, noise)
        return process_x0(xi)

    return sample


def _nullspace_operator(likelihood, xT):
    """The mi355_nullspace_op of a likelihood for a state of xT's shape: InPainting / OutPainting -> the mask (kind 0), AveragePooling -> the block
    mean (kind 1), LowResolution -> the bilinear taps of an integer factor (kind 2).  Anything else is refused by name."""
    name = type(likelihood).__name__
    H, W = int(xT.shape[-2]), int(xT.shape[-1])
    if hasattr(likelihood, "pad_value"):
        return default_ops.nullspace_op("mask", pad_value=float(likelihood.pad_value))
    if name == "HyperResolution":
        raise NotImplementedError("NullSpace is not built for HyperResolution: its condition is the re-enlarged image, an operator without a disjoint "
                                  "pseudo-inverse - measure with LowResolution (the low-resolution image itself) or AveragePooling")
    if name == "AveragePooling":
        fy, fx = likelihood.factor
        if H % fy or W % fx:
            raise NotImplementedError(f"NullSpace: the AveragePooling factor {likelihood.factor} does not divide the image size {(H, W)}")
        return default_ops.nullspace_op("block_mean", (xT.shape[0], xT.shape[1], H // fy, W // fx))
    if name == "LowResolution":
        hl, wl = int(likelihood.target_height), int(likelihood.target_width)
        if hl < 1 or wl < 1 or H % hl or W % wl:
            raise NotImplementedError(f"NullSpace: the LowResolution factor {(H / max(hl, 1), W / max(wl, 1))} (image {(H, W)} over target {(hl, wl)}) is "
                                      "not an integer: the rows of the bilinear reduction are disjoint for integer factors only")
        return default_ops.nullspace_op("bilinear", (xT.shape[0], xT.shape[1], hl, wl))
    raise NotImplementedError(f"NullSpace has no linear operator for likelihood {name}")


def _nullspace_sample_fn(eps_model, ddpm, conditioning: NullSpace, likelihood):
    """BUILD-DEFINED EXTENSION (no reference counterpart): DDNM (Wang, Yu, Zhang 2023) with an unconditional eps_model.  sample(xT, condition,
    y=None): condition is likelihood.sample's measurement, y optional class labels [B] of a class-conditional net (the fused path).  Per step one
    evaluation and ONE launch, the null-space step (mi355_nullspace_step): the data prediction is rectified against the measurement with
    ddpm.nullspace_coefs(sigma_y)'s lam, then the state moves by the ancestral step (eta None; its sigma from the same call) or the DDIM(eta) step
    (ddpm.ddim_sigma(eta); eta 0: deterministic, no draw).  jump_length / n_resample: the walk of DDNM's time travel.  Fused path (eps_model built by
    make_eps_model for this very schedule): the whole loop in mi355_ddpm_nullspace_sample; any other callable: a host loop over nullspace_step_.
    x0- and v-prediction chains and respaced chains are taken; a learned-variance chain in the DDIM form only.  Sample quality is untested."""
    form = 0 if conditioning.eta is None else 1
    sigma_y = float(conditioning.sigma_y)
    if form == 1 and sigma_y > 0.0:
        raise ValueError("sigma_y > 0 (DDNM+) belongs to the ancestral form (eta=None): the DDIM form has no closed-form noise split here")
    if getattr(ddpm, "x0_shaping", None) is not None:
        raise NotImplementedError("x0 shaping (DDPM.with_x0_shaping) is not built for NullSpace: the rectification works on the statically clipped x0_hat")
    if getattr(ddpm, "learned_variance", False) and form == 0:
        raise NotImplementedError("a learned-variance chain (DDPM.with_learned_variance) is taken by NullSpace in the DDIM form only (eta=): its "
                                  "learned variance and DDNM+'s are not reconciled")
    if _custom_times(ddpm) is not None:
        raise NotImplementedError("NullSpace is not built for a chain with a time_scale (DDPM.from_betas(..., time_scale=))")
    for what in ("n_corrector", "guidance_scale", "order"):   # correctors, classifier-free guidance, multistep solvers: not parameters of NullSpace
        if getattr(conditioning, what, None):
            raise NotImplementedError(f"{what} is not built for NullSpace")
    pred = _pred_of(ddpm)
    wide = bool(getattr(ddpm, "learned_variance", False))
    lam, sig = ddpm.nullspace_coefs(sigma_y)
    dsig = ddpm.ddim_sigma(float(conditioning.eta)) if form == 1 and float(conditioning.eta) != 0.0 else None
    walk = repaint_walk(ddpm.Ns, conditioning.jump_length, conditioning.n_resample)
    if all(b < a for a, b in zip(walk, walk[1:])):
        walk = None

    @torch.no_grad()
    def sample(xT, condition, y=None):
        global _draw_counter
        T = _tables(ddpm)
        op = _nullspace_operator(likelihood, xT)
        condition = condition.to(xT.device).float().contiguous()
        xi = xT.detach().clone().float().contiguous()
        engine = _fast_engine(eps_model, ddpm, xT)
        if engine is not None:
            out_channels = getattr(engine, "out_channels", None)
            if out_channels is not None:
                _check_width(out_channels, xi, True if wide else None)
            noise, seed = None, int(torch.initial_seed()) & ((1 << 63) - 1)
            if _injected is not None:
                noise = torch.stack([z.to(xi.device, torch.float32) for z in _injected]).contiguous()
            else:
                seed = (seed + 0x9E3779B97F4A7C15 * (_draw_counter + 1)) & ((1 << 63) - 1)
                _draw_counter += 1
            sched = {}
            if getattr(ddpm, "timesteps", None) is not None or dsig is not None or walk is not None:
                sched = dict(timesteps=getattr(ddpm, "timesteps", None) or tuple(range(ddpm.Ns)), train_steps=int(getattr(ddpm, "base_Ns", ddpm.Ns)),
                             ddim_sigma=dsig, walk=walk)
            engine.ddpm_nullspace(xi, T, condition, op, lam, sig if form == 0 else None, mode=_lib.DDIM if form else _lib.DDPM_PRIOR, prediction=pred,
                                  labels=y, noise=noise, seed=seed, **sched)
            return xi
        if y is not None:
            raise NotImplementedError("class labels run inside the fused loop: pass an eps_model built by make_eps_model(network, ddpm) for this "
                                      "schedule and device tensors (an arbitrary callable takes (x, i) alone)")
        noise = _Noise(xi)
        for level, down in _walk_moves(ddpm.Ns, walk):
            if not down:   # q(x_level+1 | x_level): one draw
                z, ph = noise.next()
                _ops.renoise_(xi, z, float(T["alphas"][level].sqrt()), float(T["betas"][level].sqrt()), ph)
                continue
            i = level - 1
            out = eps_model(xi, _times(xi, i)).float().contiguous()
            _check_width(out.shape[1], xi, True if wide else None)
            cr, crm1 = float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i])
            if form == 0:
                z, ph = noise.next() if i > 0 else (None, None)
                _ops.nullspace_step_(op, 0, pred, xi, out, condition, cr, crm1, float(T["posterior_mean_coef1"][i]), float(T["posterior_mean_coef2"][i]),
                                     lam=float(lam[i]), sigma=float(sig[i]), z=z, philox=ph, **_pred_kw(T, i))
            else:
                z, ph = noise.next() if (dsig is not None and i > 0) else (None, None)
                _ops.nullspace_step_(op, 1, pred, xi, out, condition, cr, crm1, float(T["alphas_cumprod_prev"][i]), lam=float(lam[i]),
                                     sigma=float(dsig[i]) if dsig is not None else 0.0, z=z, philox=ph, **_pred_kw(T, i))
        return process_x0(xi)

    return sample


def _replacement_sample_fn(eps_model, ddpm, conditioning: Replacement, likelihood, walk=None, feature_cache=None, tiling=None):
    """sampling.py:209-260: overwrite the known pixels with the (noised) condition before each predictor step.
    walk (RePaint; None: the plain descent): the levels to visit, conditioning.repaint_walk; a move up re-noises the state by
    q(x_k | x_{k-1}) (mi355_renoise_step), a move down is the replacement step of its level.  A walk without upward moves is the plain descent."""
    if walk is not None and all(b < a for a, b in zip(walk, walk[1:])):
        walk = None

    @torch.no_grad()
    def sample(xT, condition):
        condition = condition.to(xT.device).float().contiguous()
        pad = float(likelihood.pad_value)
        engine = _fast_engine(eps_model, ddpm, xT)
        _need_fused(engine, feature_cache)
        _need_fused_tiling(engine, tiling)
        if engine is not None:
            return _run_fast(engine, ddpm, xT, _lib.DDPM_REPLACEMENT, condition, n_corrector=conditioning.n_corrector,
                             delta=conditioning.delta, start_fraction=conditioning.start_fraction,
                             noise_condition=conditioning.noise, pad_value=pad, walk=walk, feature_cache=feature_cache, tiling=tiling)
        rep = dict(condition=condition, start_fraction=conditioning.start_fraction, noise=bool(conditioning.noise), pad_value=pad)
        return _run_generic(eps_model, ddpm, xT, amortized=False, cond_pred=None, cond_corr=None, replacement=rep,
                            n_corrector=conditioning.n_corrector, delta=conditioning.delta, walk=walk)

    return sample


def get_dpm_solver_sample_fn(eps_model: Callable, ddpm: DDPM, likelihood: Optional[Likelihood] = None, guidance_scale=None, order=2):
    """BUILD-DEFINED EXTENSION (no reference counterpart): DPM-Solver++ multistep (Lu et al. 2022, Algorithm 2) of order 1 or 2 on the same tables,
    in the data-prediction form with the reference's clipped x0_hat.  sample(xT, condition=None), deterministic, one evaluation per step like
    get_ddim_sample_fn; order 1 is the deterministic DDIM step written with other coefficients, order 2 reuses the previous step's data
    prediction.  The coefficients are ddpm.dpm_solver_coefs(order); the second order pays on steps spaced evenly in logSNR:
    ddpm.respace(ddpm.logsnr_steps(K)).  guidance_scale (None: unguided): classifier-free guidance of eps against the none_like condition; needs
    a condition.  Fused path (eps_model built by make_eps_model for this very schedule): the whole loop in mi355_ddpm_multistep_sample; any other
    callable: a host loop over dpmpp_step_ (guided: cfg_combine, then the step).  Sample quality is untested."""
    _refuse_feature_cache(_cache_of(ddpm), "the DPM-Solver++ multistep loops")
    _refuse_tiling(_tiling_of(ddpm), "the DPM-Solver++ multistep loops")
    coefs = ddpm.dpm_solver_coefs(order)
    cx, c0, c1 = (c.tolist() for c in coefs)
    shaping = _shaping_of(ddpm, guidance_scale is not None)
    max_log = _learned_of(ddpm)   # a learned-variance chain: the solver reads the eps channels of the 2C output
    pred = _pred_of(ddpm)
    times = _custom_times(ddpm)

    @torch.no_grad()
    def sample(xT, condition=None):
        T = _tables(ddpm)
        engine = _fast_engine(eps_model, ddpm, xT)
        if condition is not None:
            condition = condition.to(xT.device).float().contiguous()
        if guidance_scale is not None and condition is None:
            raise ValueError("guidance_scale needs a condition to guide towards")
        xi = xT.detach().clone().float().contiguous()
        if engine is not None:
            nv = _none_value(likelihood, xT) if likelihood is not None else 0.0
            sched = {}
            if getattr(ddpm, "timesteps", None) is not None:
                sched = dict(timesteps=ddpm.timesteps, train_steps=int(ddpm.base_Ns))
            if pred != "eps":
                _check_engine_width(engine, xi, max_log)
                return engine.ddpm_pred(xi, T, pred, shaping=shaping, max_log=max_log, times=times, mode=_lib.DDIM, coefs=coefs, cond=condition,
                                        none_value=nv, guidance_scale=guidance_scale, **sched)
            if max_log is not None or times is not None:
                if shaping is not None:
                    raise NotImplementedError("x0_shaping is not built for a chain with a time_scale (DDPM.from_betas(..., time_scale=))")
                _check_engine_width(engine, xi, max_log)
                return engine.ddpm_learned(xi, T, max_log, times=times, mode=_lib.DDIM, coefs=coefs, cond=condition, none_value=nv,
                                           guidance_scale=guidance_scale, **sched)
            if shaping is not None:
                return engine.ddpm_shaped(xi, T, shaping, mode=_lib.DDIM, coefs=coefs, cond=condition, none_value=nv, guidance_scale=guidance_scale,
                                          **sched)
            return engine.ddpm_multistep(xi, T, coefs, cond=condition, none_value=nv, guidance_scale=guidance_scale, **sched)
        none = None
        if guidance_scale is not None:
            none = likelihood.none_like(xT) if likelihood is not None else torch.zeros_like(condition)
        hist = torch.empty_like(xi)
        for i in reversed(range(ddpm.Ns)):
            eps = eps_model(_net_in(xi, condition, condition is not None), _times(xi, i)).float().contiguous()
            shape = None
            _check_width(eps.shape[1], xi, max_log, host_loop=True)
            cr, crm1 = float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i])
            if pred != "eps":   # the raw output of an x0- or v-prediction net, passed whole (guided: the pair, on the duplicated state)
                if none is None:
                    _ops.pred_step_("dpmpp", pred, xi, eps, cr, crm1, cx[i], c0[i], c1[i], hist=hist,
                                    shape=_shape_rows(xi, eps, i, T, shaping, pred=pred), **_pred_kw(T, i))
                    continue
                eps2 = torch.cat((eps, eps_model(_net_in(xi, none, True), _times(xi, i)).float())).contiguous()
                x2 = torch.cat((xi, xi))
                _ops.pred_step_("dpmpp", pred, x2, eps2, cr, crm1, cx[i], c0[i], c1[i], hist=hist, w=guidance_scale,
                                shape=_shape_rows(xi, eps2, i, T, shaping, w=guidance_scale, pred=pred), **_pred_kw(T, i))
                xi.copy_(x2[:xi.shape[0]])
                continue
            if max_log is not None:   # the 2C output, passed whole (guided: the pair, on the duplicated state)
                if none is None:
                    _ops.strided_step_("dpmpp", xi, eps, cr, crm1, cx[i], c0[i], c1[i], hist=hist)
                    continue
                eps2 = torch.cat((eps, eps_model(_net_in(xi, none, True), _times(xi, i)).float())).contiguous()
                x2 = torch.cat((xi, xi))
                _ops.strided_step_("dpmpp", x2, eps2, cr, crm1, cx[i], c0[i], c1[i], hist=hist, w=guidance_scale)
                xi.copy_(x2[:xi.shape[0]])
                continue
            if none is not None:
                eu = eps_model(_net_in(xi, none, True), _times(xi, i)).float()
                eps2 = torch.cat((eps, eu)).contiguous()
                shape = _shape_rows(xi, eps2, i, T, shaping, w=guidance_scale)
                eps = _ops.cfg_combine(eps2, guidance_scale)
            else:
                shape = _shape_rows(xi, eps, i, T, shaping)
            if shape is not None:
                _ops.x0_shaped_step_("dpmpp", xi, eps, shape, cr, crm1, cx[i], c0[i], c1[i], hist=hist)
            else:
                _ops.dpmpp_step_(xi, eps, hist, cr, crm1, cx[i], c0[i], c1[i])
        return process_x0(xi)

    return sample


def get_ddim_sample_fn(eps_model: Callable, ddpm: DDPM, likelihood: Optional[Likelihood] = None, guidance_scale=None, eta=0.0):
    """BUILD-DEFINED EXTENSION (no reference counterpart; BASELINE.json configs 3/5 name DDIM): deterministic
    DDIM(eta=0) on the same tables with the reference's clipped x0_hat.  sample(xT, condition=None).
    guidance_scale (None: unguided): classifier-free guidance of eps against the none_like condition; needs a condition.
    eta (0: the deterministic sampler, untouched): stochastic DDIM with sigma = ddpm.ddim_sigma(eta), one noise draw per step with i > 0;
    eta = 1 has the ancestral step's mean and variance.  On a RespacedDDPM this is DDIM on a sub-sequence of the training steps.
    On a chain that carries a Tiling (ddpm.with_tiling(Tiling(...))) xT (and the condition) are canvases.  Not with guidance_scale."""
    tiling = _tiling_of(ddpm)
    if guidance_scale is not None:
        _refuse_tiling(tiling, "the guided (classifier-free guidance) loops")
    feature_cache = _cache_of(ddpm)   # DDPM.with_feature_cache: feature reuse across the steps (the fused path only; not under guidance)
    if guidance_scale is not None:
        _refuse_feature_cache(feature_cache, "the guided (classifier-free guidance) loops")
    eta = float(eta)
    if not (math.isfinite(eta) and eta >= 0.0):
        raise ValueError(f"eta must be finite and >= 0, got {eta!r}")
    sigma = ddpm.ddim_sigma(eta) if eta != 0.0 else None
    shaping = _shaping_of(ddpm, guidance_scale is not None)
    max_log = _learned_of(ddpm, tiling=tiling, feature_cache=feature_cache)
    pred = _pred_of(ddpm, tiling=tiling, feature_cache=feature_cache)

    @torch.no_grad()
    def sample(xT, condition=None):
        T = _tables(ddpm)
        engine = _fast_engine(eps_model, ddpm, xT)
        if condition is not None:
            condition = condition.to(xT.device).float().contiguous()
        if guidance_scale is not None and condition is None:
            raise ValueError("guidance_scale needs a condition to guide towards")
        _need_fused(engine, feature_cache)
        _need_fused_tiling(engine, tiling)
        if engine is not None:
            nv = _none_value(likelihood, xT) if likelihood is not None else 0.0
            return _run_fast(engine, ddpm, xT, _lib.DDIM, condition, none_value=nv, guidance_scale=guidance_scale, ddim_sigma=sigma,
                             feature_cache=feature_cache, tiling=tiling)
        if guidance_scale is not None:
            none = likelihood.none_like(xT) if likelihood is not None else torch.zeros_like(condition)
            return _run_generic_cfg(eps_model, ddpm, xT, cond=condition, none=none, guidance_scale=guidance_scale, ddim=True, ddim_sigma=sigma)
        xi = xT.detach().clone().float().contiguous()
        noise = _Noise(xi) if sigma is not None else None
        for i in reversed(range(ddpm.Ns)):
            eps = eps_model(_net_in(xi, condition, condition is not None), _times(xi, i)).float().contiguous()
            _check_width(eps.shape[1], xi, max_log, host_loop=True)
            _ddim_move(eps, xi, i, T, sigma, noise, _shape_rows(xi, eps, i, T, shaping, pred=pred), wide=max_log is not None, pred=pred)
        return process_x0(xi)

    return sample
