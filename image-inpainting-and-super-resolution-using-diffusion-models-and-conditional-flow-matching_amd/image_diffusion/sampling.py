"""Counterpart of `AD/image_diffusion/sampling.py`: the reverse-denoising samplers.

Same factories and call contracts as the reference:
    get_prior_sample_fn(eps_model, ddpm, conditioning, likelihood)        -> sample(xT)
    get_conditional_sample_fn(eps_model, ddpm, conditioning, likelihood)  -> sample(xT, condition)
`eps_model(xi, i)` takes a long [B] step-index tensor (experiments/main.py:140).  Dispatch is on
`type(conditioning)` (the reference uses the un-vendored `plum` package for that).
Build-defined extensions without a reference counterpart: get_ddim_sample_fn (DDIM(eta)), get_dpm_solver_sample_fn (DPM-Solver++ multistep, orders
1 and 2), the ClassifierFreeGuidance, RePaint and NullSpace conditionings, FeatureCache and Tiling; sample quality of all of them is untested.

Every factory reads the chain's form once (_chain_form: what the net's output stands for, the learned variance range, per-image x0 shaping, the
chain's own times, tiling, feature cache; DDPM.with_prediction, with_learned_variance, with_x0_shaping, from_betas, with_tiling,
with_feature_cache) and refuses there, by name, what is not built for it.  Two execution paths, both entirely on the HIP backend:
  * fused - `eps_model` was made by `make_eps_model(network, ddpm)` with a `UNetModel` for this very schedule: the whole loop runs inside
    libmi355_sampler, one C call per sample() call.  _fused_operands prepares the state, the injected draws or the call's Philox seed and the
    schedule; _fused_call picks the engine method from the chain's form (ddpm_pred, ddpm_learned, ddpm_shaped, else ddpm_sample or
    ddpm_multistep); the null-space sampler calls ddpm_nullspace on the same operands.
  * host loop - any callable `eps_model` (e.g. the reference's own lambda around a UNetModel): ONE loop, _run_host, walks the chain (a RePaint
    walk re-noises on its upward moves), pastes the replacement's known pixels, evaluates the eps_model, takes the predictor step of the sampler's
    kind and the Langevin correctors, and clips.  ONE dispatch, _step, maps (step kind, chain form) to the fused HIP step kernel
    (csrc/steps.hip) and makes the step's noise draw: kinds "ddpm", "ddim", "ddim_eta", "dpmpp", "corrector" and "nullspace"; a plain chain
    takes the kind's own op, a shaped one x0_shaped_step_ on the rows of _shape_rows, a learned-variance one strided_step_ / ddpm_lv_step_ on
    the net's 2C output as it is, an x0- or v-prediction one pred_step_ on the raw output.  Under guidance the loop evaluates the condition,
    then `none`, and takes one of two forms: combine then plain step (cfg_combine, then the unguided step on the state: eps chains without a
    learned variance), or the pair on the duplicated state (the guided step kernel on cat(xi, xi) with the raw [2B] pair: learned variance, x0
    and v prediction).
Noise: by default drawn in-kernel (Philox4x32-10, seeded from torch.initial_seed()); parity tests
inject the draws of the reference's `torch.randn_like` call sequence with `injected_noise([...])`.
ReconstructionGuidance (sampling.py:136-206) differentiates the x0 model through the U-Net: the gradient is the HIP engine's
vector-Jacobian product (`UNetEngine.vjp`, csrc/unet_backward.hip) of a differentiable plan of the same network, so it needs an
`eps_model` made by `make_eps_model(network, ddpm)` around a `UNetModel`; its loop (two engines, the VJP between evaluation and step) is its
own and takes its predictor and corrector from _step.
"""
from __future__ import annotations

import contextlib
import math
from typing import Callable, List, NamedTuple, Optional

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
    eps_model(xi, i) = network(xi, tau_i / base_Ns), for an int i and for the long [B] tensor the samplers pass.  The name stays on an x0- or
    v-prediction chain: the model returns whatever the net writes."""
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


# The chain's form ---------------------------------------------------------------------------------------

class _Form(NamedTuple):
    """What a factory reads off its chain, once."""
    pred: str                   # what the net's output stands for: "eps", "x0" or "v" (DDPM.with_prediction)
    max_log: Optional[torch.Tensor]   # ddpm.max_log() of a learned-variance chain (DDPM.with_learned_variance), else None
    shaping: object             # ddpm.x0_shaping (DDPM.with_x0_shaping), None on a plain chain
    times: Optional[torch.Tensor]     # the K times the net sees where the chain's time_scale is not 1 (DDPM.from_betas), else None
    tiling: object              # the factory's argument, else the chain's (DDPM.with_tiling)
    feature_cache: object       # the factory's argument, else the chain's (DDPM.with_feature_cache)

    @property
    def wide(self) -> bool:
        """The net writes 2C channels (eps | v), passed whole to the step ops."""
        return self.max_log is not None


def _need_guided(form: _Form, guided: bool):
    if form.shaping is not None and form.shaping.guidance_rescale > 0.0 and not guided:
        raise ValueError("guidance_rescale > 0 rescales the guided eps against the conditional one: it needs a guided sampler "
                         "(ClassifierFreeGuidance, or guidance_scale=)")


def _chain_form(ddpm, *, guided=None, tiling=None, feature_cache=None) -> _Form:
    """The chain's form with the refusals, by name, of what is not built for it.  guided (None: not known before sample()): the guidance
    rescale needs a guided sampler, _need_guided."""
    pred = getattr(ddpm, "prediction", "eps")
    learned = bool(getattr(ddpm, "learned_variance", False))
    form = _Form(pred, ddpm.max_log() if learned else None, getattr(ddpm, "x0_shaping", None), _custom_times(ddpm),
                 tiling if tiling is not None else getattr(ddpm, "tiling", None),
                 feature_cache if feature_cache is not None else getattr(ddpm, "feature_cache", None))
    if guided is not None:
        _need_guided(form, guided)
    def whole_frames_only(chain):
        for what, v in (("tiling", form.tiling), ("feature_cache", form.feature_cache)):
            if v is not None:
                raise NotImplementedError(f"{what} is not built for {chain}")

    if learned:
        if form.shaping is not None:
            raise NotImplementedError("per-image x0_shaping (DDPM.with_x0_shaping) is not built for a learned-variance chain (DDPM.with_learned_variance)")
        whole_frames_only("a learned-variance chain (DDPM.with_learned_variance)")
        if getattr(ddpm, "fixed_variance", "small") == "large":   # which of the two variances is meant?
            raise NotImplementedError('a fixed variance (DDPM.with_fixed_variance("large")) is not built for a learned-variance chain '
                                      "(DDPM.with_learned_variance): the chain has one variance")
    if pred != "eps":
        whole_frames_only("an x0- or v-prediction chain (DDPM.with_prediction)")
    return form


def _refuse(loop: str, **what):
    """tiling= / feature_cache= (checked in the order given) where the loop takes neither."""
    for name, v in what.items():
        if v is not None:
            raise NotImplementedError(f"{name} is not built for {loop} (it runs with the prior, amortized, replacement / RePaint and DDIM samplers)")


class _Coefs(NamedTuple):
    """The floats of step i, each from the fp32 host tables."""
    i: int
    c_recip: float
    c_recipm1: float
    coef1: float
    coef2: float
    sigma: float      # exp(0.5 * posterior log-variance), in fp32 like the reference's (0.5 * logvar).exp()
    acp_prev: float
    sa: float         # sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod: the paste, and the "v" kind's data prediction
    sb: float
    min_log: float    # the clipped posterior log-variance: the lower end of a learned variance range
    rsm1: float


def _coefs(T, i) -> _Coefs:
    return _Coefs(i, float(T["sqrt_recip_alphas_cumprod"][i]), float(T["sqrt_recipm1_alphas_cumprod"][i]), float(T["posterior_mean_coef1"][i]),
                  float(T["posterior_mean_coef2"][i]), float((0.5 * T["posterior_log_variance_clipped"][i]).exp()),
                  float(T["alphas_cumprod_prev"][i]), float(T["sqrt_alphas_cumprod"][i]), float(T["sqrt_one_minus_alphas_cumprod"][i]),
                  float(T["posterior_log_variance_clipped"][i]), float(T["recip_sqrt_m1_alphas_cumprod"][i]))


def _shape_rows(xi, out, c: _Coefs, form: _Form, w=None):
    """The per-image rows (f, s) of the step's shaped data prediction, or None without shaping.  w: out is the [2B] pair of a guided step (the
    rescale needs eps_c beside eps_g)."""
    if form.shaping is None:
        return None
    if form.pred != "eps":
        return _ops.pred_shape_stats(form.pred, xi, out, c.c_recip, c.c_recipm1, form.shaping, w=w, sa=c.sa, sb=c.sb)
    return _ops.x0_shape_stats(xi, out, c.c_recip, c.c_recipm1, form.shaping, w=w)


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


def _step(kind, xi, out, c: _Coefs, form: _Form, noise: _Noise, args=(), *, w=None, hist=None, shape=None):
    """One step of `kind` in place on xi from the net's output `out`, with the kind's noise draw (before anything else):
        "ddpm"       step() (sampling.py:59-67): x0_hat -> clip -> posterior mean -> + sigma z; one draw iff i > 0
        "ddim"       the deterministic DDIM step
        "ddim_eta"   args = (sigma_i,): DDIM(eta); one draw iff i > 0
        "dpmpp"      args = (cx_i, c0_i, c1_i): DPM-Solver++ multistep on hist, the previous step's data prediction
        "corrector"  args = (dt, delta): corrector_step (sampling.py:113-121); one draw
        "nullspace"  args = (op, form, y, lam_i, sigma_i or None): the null-space step, ancestral (form 0) or DDIM(eta) (form 1; None: no draw)
    The chain's form picks the op: a plain chain the kind's own; shape (the rows of _shape_rows, per-image shaping in place of the clip)
    x0_shaped_step_; a learned-variance chain strided_step_ on the 2C output passed whole, ddpm_lv_step_ where the learned variance is drawn
    with (the ancestral step, i > 0; step 0 draws no noise and never reads v); an x0- or v-prediction chain pred_step_ on the raw output.
    w: out is the [2B] pair of a guided step and xi the duplicated state."""
    cr, crm1 = c.c_recip, c.c_recipm1
    if kind == "nullspace":
        op, ns_form, y, lam, sigma = args
        z, ph = noise.next() if (sigma is not None and c.i > 0) else (None, None)
        a, b = (c.coef1, c.coef2) if ns_form == 0 else (c.acp_prev, 0.0)
        return _ops.nullspace_step_(op, ns_form, form.pred, xi, out, y, cr, crm1, a, b, lam=lam, sigma=0.0 if sigma is None else sigma, z=z,
                                    philox=ph, sa=c.sa, sb=c.sb)
    z, ph = noise.next() if (kind == "corrector" or (kind in ("ddpm", "ddim_eta") and c.i > 0)) else (None, None)
    b = cc = sigma = 0.0   # the ops' three numbers a, b, c of the kind, and its sigma
    if kind == "ddpm":
        a, b, sigma = c.coef1, c.coef2, c.sigma
    elif kind == "ddim":
        a = c.acp_prev
    elif kind == "ddim_eta":
        a, (sigma,) = c.acp_prev, args
    elif kind == "dpmpp":
        a, b, cc = args
    else:
        a, (b, cc) = c.rsm1, args
    lv = form.wide and kind == "ddpm" and c.i > 0
    lo, hi = (c.min_log, float(form.max_log[c.i])) if lv else (0.0, 0.0)   # the learned range, in place of sigma
    if form.pred != "eps":
        return _ops.pred_step_("ddpm_lv" if lv else kind, form.pred, xi, out, cr, crm1, a, b, cc, 0.0 if lv else sigma, sa=c.sa, sb=c.sb, min_log=lo,
                               max_log=hi, z=z, philox=ph, hist=hist, w=w, shape=shape)
    if lv:
        return _ops.ddpm_lv_step_(xi, out, z, cr, crm1, a, b, lo, hi, ph, w=w)
    if form.wide:
        return _ops.strided_step_(kind, xi, out, cr, crm1, a, b, cc, sigma, z=z, philox=ph, hist=hist, w=w)
    if shape is not None:
        return _ops.x0_shaped_step_(kind, xi, out, shape, cr, crm1, a, b, cc, sigma, z=z, philox=ph, hist=hist)
    if kind == "ddpm":
        return _ops.ddpm_step_(xi, out, z, cr, crm1, a, b, sigma, ph)
    if kind == "ddim":
        return _ops.ddim_step_(xi, out, cr, crm1, a)
    if kind == "ddim_eta":
        return _ops.ddim_eta_step_(xi, out, z, cr, crm1, a, sigma, ph)
    if kind == "dpmpp":
        return _ops.dpmpp_step_(xi, out, hist, cr, crm1, a, b, cc)
    return _ops.corrector_step_(xi, out, z, cr, crm1, a, b, cc, ph)


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


def _run_host(eps_model, ddpm, xT, form: _Form, kind="ddpm", step_args=lambda i: (), *, cond=None, concat=False, none=None, w=None, cond_corr=None,
              replacement=None, n_corrector=0, delta=0.1, walk=None):
    """The host loop for any eps_model callable.  Per move of the walk (None: the plain descent): an upward move re-noises the state by
    q(x_level+1 | x_level) (one draw); a downward move pastes the replacement's known pixels (one draw iff they are noised), evaluates the net
    on cond (concatenated iff concat), takes the predictor step of `kind` (_step; step_args(i): the kind's own numbers) and n_corrector
    correctors, each on an evaluation on cond_corr.  w (a float or a [B] tensor; None: unguided): classifier-free guidance, a second evaluation
    on `none` behind the conditional one, the width check on the pair, the shaping rows from the pair, and one of two forms - the pair on the
    duplicated state where the step kernel must see it raw (a 2C pair: v from the conditional half; an x0- or v-prediction pair: mixed raw),
    else cfg_combine and the unguided step."""
    _need_guided(form, w is not None)
    T = _tables(ddpm)
    xi = xT.detach().clone().float().contiguous()
    noise = _Noise(xi)
    hist = torch.empty_like(xi) if kind == "dpmpp" else None
    dt = (ddpm.tmax - ddpm.tmin) / ddpm.Ns
    for level, down in _walk_moves(ddpm.Ns, walk):
        if not down:   # q(x_level+1 | x_level): one draw
            z, ph = noise.next()
            _ops.renoise_(xi, z, float(T["alphas"][level].sqrt()), float(T["betas"][level].sqrt()), ph)
            continue
        i = level - 1
        c = _coefs(T, i)
        if replacement is not None and i < int(ddpm.Ns * replacement["start_fraction"]):
            z, ph = noise.next() if replacement["noise"] else (None, None)
            _ops.replace_mask_(xi, replacement["condition"], z, replacement["pad_value"], replacement["noise"], c.sa, c.sb, ph)
        out = eps_model(_net_in(xi, cond, concat), _times(xi, i)).float()
        if w is not None:
            out = torch.cat((out, eps_model(_net_in(xi, none, True), _times(xi, i)).float()))
        out = out.contiguous()
        _check_width(out.shape[1], xi, form.max_log, host_loop=kind != "nullspace")
        shape = _shape_rows(xi, out, c, form, w=w)
        if w is None:
            _step(kind, xi, out, c, form, noise, step_args(i), hist=hist, shape=shape)
        elif form.wide or form.pred != "eps":
            x2 = torch.cat((xi, xi))
            _step(kind, x2, out, c, form, noise, step_args(i), w=w, hist=hist, shape=shape)
            xi.copy_(x2[:xi.shape[0]])
        else:
            _step(kind, xi, _ops.cfg_combine(out, w), c, form, noise, step_args(i), hist=hist, shape=shape)
        for _ in range(n_corrector):
            out = eps_model(_net_in(xi, cond_corr, concat), _times(xi, i))
            _step("corrector", xi, out.float().contiguous(), c, form, noise, (dt, float(delta)))
    return process_x0(xi)


def _run_generic_cfg(eps_model, ddpm, xT, *, cond, none, guidance_scale, n_corrector=0, delta=0.1, ddim=False, ddim_sigma=None):
    """The guided host loop under its earlier name and signature: _run_host with (none, w); ddim: the DDIM(eta) kinds, no correctors."""
    kind, step_args = ("ddpm", lambda i: ()) if not ddim else ("ddim", lambda i: ()) if ddim_sigma is None else ("ddim_eta", lambda i: (float(ddim_sigma[i]),))
    form = _chain_form(ddpm.with_tiling(None).with_feature_cache(None), guided=True)   # (tiling and cache are the factories' to refuse)
    return _run_host(eps_model, ddpm, xT, form, kind, step_args, cond=cond, concat=True, none=none, w=guidance_scale,
                     cond_corr=none, n_corrector=0 if ddim else n_corrector, delta=delta)


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


# The fused path: one preparation, one choice of the engine method ----------------------------------------------------

def _fused_operands(ddpm, xT, *, ddim_sigma=None, walk=None, draws=True):
    """-> (xi, noise, seed, sched) of a fused call: the state; the injected draws stacked, or None and the call's Philox seed, keyed with
    _draw_counter; the keywords of the scheduled entry points - a respaced chain's steps in training time (an unrespaced one's: 0..Ns-1 of Ns),
    the DDIM sigma and the walk - where the call has any of them.  draws=False (a deterministic multistep call): no noise, no seed, no key
    taken, and a schedule of the steps alone."""
    global _draw_counter
    xi = xT.detach().clone().float().contiguous()
    noise, seed = None, None
    if draws:
        seed = int(torch.initial_seed()) & ((1 << 63) - 1)
        if _injected is not None:
            noise = torch.stack([z.to(xi.device, torch.float32) for z in _injected]).contiguous()
        else:
            seed = (seed + 0x9E3779B97F4A7C15 * (_draw_counter + 1)) & ((1 << 63) - 1)
            _draw_counter += 1
    sched = {}
    if getattr(ddpm, "timesteps", None) is not None or ddim_sigma is not None or walk is not None:
        sched = dict(timesteps=getattr(ddpm, "timesteps", None) or tuple(range(ddpm.Ns)), train_steps=int(getattr(ddpm, "base_Ns", ddpm.Ns)))
        if draws:
            sched.update(ddim_sigma=ddim_sigma, walk=walk)
    return xi, noise, seed, sched


def _fused_call(engine, ddpm, xi, form: _Form, kw, coefs=None):
    """The engine method of the chain's form, on the keywords kw every one of them takes: ddpm_pred (an x0- or v-prediction net; it takes the
    shaping, the variance range and the times beside the kind), ddpm_learned (a learned variance range and / or the chain's own times),
    ddpm_shaped (per-image shaping of x0_hat), else ddpm_sample - or, with coefs (DPM-Solver++), ddpm_multistep, the first three in their
    multistep form.  -> xi"""
    T = _tables(ddpm)
    guided = kw.get("guidance_scale") is not None
    multistep = {} if coefs is None else dict(mode=_lib.DDIM, coefs=coefs)
    if coefs is None or form.pred != "eps" or form.max_log is not None or form.times is not None:
        _check_engine_width(engine, xi, form.max_log)   # (ddpm_multistep and its shaped form leave a plain chain's width to the library)
    if form.pred != "eps":
        engine.ddpm_pred(xi, T, form.pred, shaping=form.shaping, max_log=form.max_log, times=form.times, **multistep, **kw)
        return xi
    for name, v in (("feature_cache", form.feature_cache), ("tiling", form.tiling)):
        if guided:
            _refuse("the guided (classifier-free guidance) loops", **{name: v})
        if form.shaping is not None:
            _refuse("the shaped loops (DDPM.with_x0_shaping)", **{name: v})
    if form.feature_cache is not None and form.tiling is not None:
        raise NotImplementedError("tiling together with feature_cache is not built")
    if form.feature_cache is not None:
        kw = dict(kw, **form.feature_cache.kwargs())
    if form.tiling is not None:
        kw = dict(kw, tiling=form.tiling)
    if form.max_log is not None or form.times is not None:
        for what, v in (("x0_shaping", form.shaping), ("tiling", form.tiling), ("feature_cache", form.feature_cache)):
            if v is not None:
                raise NotImplementedError(f"{what} is not built for a chain with a time_scale (DDPM.from_betas(..., time_scale=))")
        engine.ddpm_learned(xi, T, form.max_log, times=form.times, **multistep, **kw)
    elif form.shaping is not None:
        engine.ddpm_shaped(xi, T, form.shaping, **multistep, **kw)
    elif coefs is not None:
        engine.ddpm_multistep(xi, T, coefs, **kw)
    else:
        engine.ddpm_sample(xi, T, **kw)
    return xi


def _run_fast(engine, ddpm, xT, mode, cond, *, n_corrector=0, delta=0.1, start_fraction=1.0, noise_condition=True,
              pad_value=-2.0, none_value=-2.0, guidance_scale=None, ddim_sigma=None, walk=None, feature_cache=None, tiling=None):
    """One fused call of the noise-drawing loops; the chain's form is read here, with the caller's feature_cache= and tiling=."""
    xi, noise, seed, sched = _fused_operands(ddpm, xT, ddim_sigma=ddim_sigma, walk=walk)
    kw = dict(mode=mode, cond=cond, noise=noise, n_corrector=n_corrector, delta=float(delta), tmin=ddpm.tmin, tmax=ddpm.tmax,
              start_fraction=float(start_fraction), noise_condition=bool(noise_condition), pad_value=float(pad_value), none_value=float(none_value),
              seed=seed, guidance_scale=guidance_scale, **sched)
    form = _chain_form(ddpm, guided=guidance_scale is not None, tiling=tiling, feature_cache=feature_cache)
    return _fused_call(engine, ddpm, xi, form, kw)


def _custom_times(ddpm):
    """The K times the net sees on a chain whose time_scale is not 1 (DDPM.from_betas), None where the fused loops' own rule holds."""
    if float(getattr(ddpm, "time_scale", 1.0)) == 1.0:
        return None
    return torch.tensor([ddpm.time(k) for k in range(ddpm.Ns)], dtype=torch.float32)


def _need_fused(engine, form: _Form):
    """A feature cache and tiling run inside the fused loop only."""
    if form.feature_cache is not None and engine is None:
        raise NotImplementedError("feature_cache runs inside the fused loop: pass an eps_model built by make_eps_model(network, ddpm) for this "
                                  "schedule and device tensors (an arbitrary callable is evaluated whole)")
    if form.tiling is not None and engine is None:
        raise NotImplementedError("tiling runs inside the fused loop: pass an eps_model built by make_eps_model(network, ddpm) for this "
                                  "schedule and device tensors (an arbitrary callable sees whole frames only)")


# Prior sampling ------------------------------------------------------------------------------------

def get_prior_sample_fn(eps_model: Callable, ddpm: DDPM, conditioning: Conditioning, likelihood: Likelihood, feature_cache=None, tiling=None):
    """sampling.py:50-75.  Under Amortized conditioning the net is fed `likelihood.none_like` (sampling.py:36-37).
    feature_cache (None: untouched): a FeatureCache.  tiling (None: the chain's, ddpm.tiling; neither: untouched): a Tiling; xT is then a canvas."""
    amortized = isinstance(conditioning, Amortized)
    form = _chain_form(ddpm, tiling=tiling, feature_cache=feature_cache)   # with its refusals, before the first sample

    @torch.no_grad()
    def sample(xT):
        engine = _fast_engine(eps_model, ddpm, xT)
        _need_fused(engine, form)
        if engine is not None:
            return _run_fast(engine, ddpm, xT, _lib.DDPM_PRIOR, None, none_value=_none_value(likelihood, xT), feature_cache=form.feature_cache, tiling=form.tiling)
        none = likelihood.none_like(xT) if amortized else None
        return _run_host(eps_model, ddpm, xT, form, cond=none, concat=amortized, cond_corr=none)

    return sample


# Conditional sampling ---------------------------------------------------------------------------------

def get_conditional_sample_fn(eps_model: Callable, ddpm: DDPM, conditioning: Conditioning, likelihood: Likelihood, feature_cache=None, tiling=None):
    """feature_cache (None: the chain's, ddpm.feature_cache; neither: untouched): a FeatureCache; Amortized, Replacement and RePaint take it, the
    other conditionings refuse it by name.  tiling (None: the chain's, ddpm.tiling; neither: untouched): a Tiling, xT and the condition are then
    canvases; taken and refused by the same conditionings."""
    form = _chain_form(ddpm, tiling=tiling, feature_cache=feature_cache)   # with its refusals, before the first sample
    if isinstance(conditioning, ClassifierFreeGuidance):   # (an Amortized: before it)
        _refuse("ClassifierFreeGuidance (the guided loops)", feature_cache=form.feature_cache, tiling=form.tiling)
        return _cfg_sample_fn(eps_model, ddpm, conditioning, likelihood, form)
    if isinstance(conditioning, Amortized):
        return _amortized_sample_fn(eps_model, ddpm, conditioning, likelihood, form)
    if isinstance(conditioning, RePaint):   # (a Replacement: before it)
        return _replacement_sample_fn(eps_model, ddpm, conditioning, likelihood, form,
                                      walk=repaint_walk(ddpm.Ns, conditioning.jump_length, conditioning.n_resample))
    if isinstance(conditioning, Replacement):
        return _replacement_sample_fn(eps_model, ddpm, conditioning, likelihood, form)
    if isinstance(conditioning, NullSpace):
        _refuse("NullSpace (the null-space loop)", feature_cache=form.feature_cache, tiling=form.tiling)
        return _nullspace_sample_fn(eps_model, ddpm, conditioning, likelihood, form)
    if isinstance(conditioning, ReconstructionGuidance):
        _refuse("ReconstructionGuidance (the backward pass needs a whole forward)", feature_cache=form.feature_cache, tiling=form.tiling)
        return _reconstruction_guidance_sample_fn(eps_model, ddpm, conditioning, likelihood, form)
    raise NotImplementedError(f"no sampler for conditioning type {type(conditioning).__name__}")


def _amortized_sample_fn(eps_model, ddpm, conditioning: Amortized, likelihood, form: _Form):
    """sampling.py:80-133.  The corrector calls the x0 model WITHOUT the condition (sampling.py:116), so the
    network sees none_like there - reproduced."""

    @torch.no_grad()
    def sample(xT, condition):
        condition = condition.to(xT.device).float().contiguous()
        engine = _fast_engine(eps_model, ddpm, xT)
        _need_fused(engine, form)
        if engine is not None:
            return _run_fast(engine, ddpm, xT, _lib.DDPM_AMORTIZED, condition, n_corrector=conditioning.n_corrector,
                             delta=conditioning.delta, none_value=_none_value(likelihood, xT), feature_cache=form.feature_cache, tiling=form.tiling)
        return _run_host(eps_model, ddpm, xT, form, cond=condition, concat=True, cond_corr=likelihood.none_like(xT),
                         n_corrector=conditioning.n_corrector, delta=conditioning.delta)

    return sample


def _cfg_sample_fn(eps_model, ddpm, conditioning: ClassifierFreeGuidance, likelihood, form: _Form):
    """Amortized sampling with the predictor's eps guided: eps_u + guidance_scale * (eps_c - eps_u), eps_u from likelihood.none_like.
    Fast path: the whole loop in mi355_ddpm_cfg_sample (one forward at twice the batch per predictor step); generic path: two eps_model
    calls per predictor step (_run_host).  The corrector is the amortized sampler's."""

    @torch.no_grad()
    def sample(xT, condition):
        condition = condition.to(xT.device).float().contiguous()
        w = float(conditioning.guidance_scale)
        engine = _fast_engine(eps_model, ddpm, xT)
        if engine is not None:
            return _run_fast(engine, ddpm, xT, _lib.DDPM_AMORTIZED, condition, n_corrector=conditioning.n_corrector,
                             delta=conditioning.delta, none_value=_none_value(likelihood, xT), guidance_scale=w, feature_cache=form.feature_cache, tiling=form.tiling)
        none = likelihood.none_like(xT)
        return _run_host(eps_model, ddpm, xT, form, cond=condition, concat=True, none=none, w=w, cond_corr=none,
                         n_corrector=conditioning.n_corrector, delta=conditioning.delta)

    return sample


def _reconstruction_guidance_sample_fn(eps_model, ddpm, conditioning: ReconstructionGuidance, likelihood, form: _Form):
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
    if form.pred != "eps":
        raise NotImplementedError("ReconstructionGuidance is not built for an x0- or v-prediction chain (DDPM.with_prediction): the seed "
                                  "differentiates x0_hat = c_recip x - c_recipm1 eps of an eps net")
    if form.wide:
        raise NotImplementedError("ReconstructionGuidance is not built for a learned-variance chain (DDPM.with_learned_variance): the seed and "
                                  "the backward pass take a net that writes the state's channels")
    if form.shaping is not None:
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
        dt = (ddpm.tmax - ddpm.tmin) / ddpm.Ns
        for i in reversed(range(ddpm.Ns)):
            t = torch.full((B,), ddpm.time(i), device=xi.device, dtype=torch.float32)
            c = _coefs(T, i)
            update, eps = None, None
            if i < n_guided:
                eps = deng.forward(xi, t)
                if mode == 2:
                    g_eps, g_x, _ = _ops.lowres_seed(xi, eps, condition, c.c_recip, c.c_recipm1)
                else:
                    g_eps, g_x = _ops.guidance_seed(xi, eps, condition, c.c_recip, c.c_recipm1, mode, pad)
                vjp = deng.vjp(g_eps)
                a_i = float(alphas[i])
                scale = float(conditioning.gamma) * a_i * (1.0 - a_i)
                before = conditioning.update_rule == "before"
                update = _ops.guidance_update_(xi, g_x, vjp, scale, before)
                if before:
                    eps = None                       # xi moved: the predictor needs the network at the new point
            if eps is None:
                eps = eng.forward(xi, t)
            _step("ddpm", xi, eps, c, form, noise)
            if update is not None and conditioning.update_rule == "after":
                _ops.euler_step_(xi, update, 1.0)    # pred_img += x_update
            for _ in range(conditioning.n_corrector):
                epc = eng.forward(xi, t)
                _step("corrector", xi, epc, c, form, noise, (dt, float(conditioning.delta)))
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


def _nullspace_sample_fn(eps_model, ddpm, conditioning: NullSpace, likelihood, form: _Form):
    """BUILD-DEFINED EXTENSION (no reference counterpart): DDNM (Wang, Yu, Zhang 2023) with an unconditional eps_model.  sample(xT, condition,
    y=None): condition is likelihood.sample's measurement, y optional class labels [B] of a class-conditional net (the fused path).  Per step one
    evaluation and ONE launch, the null-space step (mi355_nullspace_step): the data prediction is rectified against the measurement with
    ddpm.nullspace_coefs(sigma_y)'s lam, then the state moves by the ancestral step (eta None; its sigma from the same call) or the DDIM(eta) step
    (ddpm.ddim_sigma(eta); eta 0: deterministic, no draw).  jump_length / n_resample: the walk of DDNM's time travel.  Fused path (eps_model built by
    make_eps_model for this very schedule): the whole loop in mi355_ddpm_nullspace_sample; any other callable: the host loop with the step kind
    "nullspace".  x0- and v-prediction chains and respaced chains are taken; a learned-variance chain in the DDIM form only.  Sample quality is
    untested."""
    ns_form = 0 if conditioning.eta is None else 1
    sigma_y = float(conditioning.sigma_y)
    if ns_form == 1 and sigma_y > 0.0:
        raise ValueError("sigma_y > 0 (DDNM+) belongs to the ancestral form (eta=None): the DDIM form has no closed-form noise split here")
    if form.shaping is not None:
        raise NotImplementedError("x0 shaping (DDPM.with_x0_shaping) is not built for NullSpace: the rectification works on the statically clipped x0_hat")
    if form.wide and ns_form == 0:
        raise NotImplementedError("a learned-variance chain (DDPM.with_learned_variance) is taken by NullSpace in the DDIM form only (eta=): its "
                                  "learned variance and DDNM+'s are not reconciled")
    if form.times is not None:
        raise NotImplementedError("NullSpace is not built for a chain with a time_scale (DDPM.from_betas(..., time_scale=))")
    for what in ("n_corrector", "guidance_scale", "order"):   # correctors, classifier-free guidance, multistep solvers: not parameters of NullSpace
        if getattr(conditioning, what, None):
            raise NotImplementedError(f"{what} is not built for NullSpace")
    lam, sig = ddpm.nullspace_coefs(sigma_y)
    dsig = ddpm.ddim_sigma(float(conditioning.eta)) if ns_form == 1 and float(conditioning.eta) != 0.0 else None
    step_sigma = sig if ns_form == 0 else dsig   # the draw's std per step; None: the deterministic DDIM form
    walk = repaint_walk(ddpm.Ns, conditioning.jump_length, conditioning.n_resample)
    if all(b < a for a, b in zip(walk, walk[1:])):
        walk = None

    @torch.no_grad()
    def sample(xT, condition, y=None):
        op = _nullspace_operator(likelihood, xT)
        condition = condition.to(xT.device).float().contiguous()
        engine = _fast_engine(eps_model, ddpm, xT)
        if engine is not None:
            out_channels = getattr(engine, "out_channels", None)
            if out_channels is not None:
                _check_width(out_channels, xT, form.max_log)
            xi, noise, seed, sched = _fused_operands(ddpm, xT, ddim_sigma=dsig, walk=walk)
            engine.ddpm_nullspace(xi, _tables(ddpm), condition, op, lam, sig if ns_form == 0 else None, mode=_lib.DDIM if ns_form else _lib.DDPM_PRIOR,
                                  prediction=form.pred, labels=y, noise=noise, seed=seed, **sched)
            return xi
        if y is not None:
            raise NotImplementedError("class labels run inside the fused loop: pass an eps_model built by make_eps_model(network, ddpm) for this "
                                      "schedule and device tensors (an arbitrary callable takes (x, i) alone)")
        return _run_host(eps_model, ddpm, xT, form, "nullspace",
                         lambda i: (op, ns_form, condition, float(lam[i]), None if step_sigma is None else float(step_sigma[i])), walk=walk)

    return sample


def _replacement_sample_fn(eps_model, ddpm, conditioning: Replacement, likelihood, form: _Form, walk=None):
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
        _need_fused(engine, form)
        if engine is not None:
            return _run_fast(engine, ddpm, xT, _lib.DDPM_REPLACEMENT, condition, n_corrector=conditioning.n_corrector,
                             delta=conditioning.delta, start_fraction=conditioning.start_fraction,
                             noise_condition=conditioning.noise, pad_value=pad, walk=walk, feature_cache=form.feature_cache, tiling=form.tiling)
        rep = dict(condition=condition, start_fraction=conditioning.start_fraction, noise=bool(conditioning.noise), pad_value=pad)
        return _run_host(eps_model, ddpm, xT, form, replacement=rep, n_corrector=conditioning.n_corrector, delta=conditioning.delta, walk=walk)

    return sample


def _guided_condition(xT, condition, guidance_scale):
    """The condition of a sample(xT, condition=None) call on the state's device; guidance needs one."""
    if condition is not None:
        condition = condition.to(xT.device).float().contiguous()
    if guidance_scale is not None and condition is None:
        raise ValueError("guidance_scale needs a condition to guide towards")
    return condition


def _guided_none(xT, condition, guidance_scale, likelihood):
    """What a guided host loop evaluates beside the condition: likelihood.none_like, zeros without a likelihood (unguided: None)."""
    if guidance_scale is None:
        return None
    return likelihood.none_like(xT) if likelihood is not None else torch.zeros_like(condition)


def get_dpm_solver_sample_fn(eps_model: Callable, ddpm: DDPM, likelihood: Optional[Likelihood] = None, guidance_scale=None, order=2):
    """BUILD-DEFINED EXTENSION (no reference counterpart): DPM-Solver++ multistep (Lu et al. 2022, Algorithm 2) of order 1 or 2 on the same tables,
    in the data-prediction form with the reference's clipped x0_hat.  sample(xT, condition=None), deterministic, one evaluation per step like
    get_ddim_sample_fn; order 1 is the deterministic DDIM step written with other coefficients, order 2 reuses the previous step's data
    prediction.  The coefficients are ddpm.dpm_solver_coefs(order); the second order pays on steps spaced evenly in logSNR:
    ddpm.respace(ddpm.logsnr_steps(K)).  guidance_scale (None: unguided): classifier-free guidance of eps against the none_like condition; needs
    a condition.  Fused path (eps_model built by make_eps_model for this very schedule): the whole loop in mi355_ddpm_multistep_sample; any other
    callable: the host loop with the step kind "dpmpp".  Sample quality is untested."""
    _refuse("the DPM-Solver++ multistep loops", feature_cache=getattr(ddpm, "feature_cache", None), tiling=getattr(ddpm, "tiling", None))
    coefs = ddpm.dpm_solver_coefs(order)
    cx, c0, c1 = (c.tolist() for c in coefs)
    form = _chain_form(ddpm, guided=guidance_scale is not None)   # (a learned-variance chain: the solver reads the eps channels of the 2C output)

    @torch.no_grad()
    def sample(xT, condition=None):
        engine = _fast_engine(eps_model, ddpm, xT)
        condition = _guided_condition(xT, condition, guidance_scale)
        if engine is not None:
            xi, _, _, sched = _fused_operands(ddpm, xT, draws=False)
            nv = _none_value(likelihood, xT) if likelihood is not None else 0.0
            return _fused_call(engine, ddpm, xi, form, dict(cond=condition, none_value=nv, guidance_scale=guidance_scale, **sched), coefs)
        return _run_host(eps_model, ddpm, xT, form, "dpmpp", lambda i: (cx[i], c0[i], c1[i]), cond=condition, concat=condition is not None,
                         none=_guided_none(xT, condition, guidance_scale, likelihood), w=guidance_scale)

    return sample


def get_ddim_sample_fn(eps_model: Callable, ddpm: DDPM, likelihood: Optional[Likelihood] = None, guidance_scale=None, eta=0.0):
    """BUILD-DEFINED EXTENSION (no reference counterpart; BASELINE.json configs 3/5 name DDIM): deterministic
    DDIM(eta=0) on the same tables with the reference's clipped x0_hat.  sample(xT, condition=None).
    guidance_scale (None: unguided): classifier-free guidance of eps against the none_like condition; needs a condition.
    eta (0: the deterministic sampler, untouched): stochastic DDIM with sigma = ddpm.ddim_sigma(eta), one noise draw per step with i > 0;
    eta = 1 has the ancestral step's mean and variance.  On a RespacedDDPM this is DDIM on a sub-sequence of the training steps.
    On a chain that carries a Tiling (ddpm.with_tiling(Tiling(...))) xT (and the condition) are canvases, on one that carries a FeatureCache
    the features are reused across the steps (both the fused path only).  Not with guidance_scale."""
    if guidance_scale is not None:
        _refuse("the guided (classifier-free guidance) loops", tiling=getattr(ddpm, "tiling", None), feature_cache=getattr(ddpm, "feature_cache", None))
    eta = float(eta)
    if not (math.isfinite(eta) and eta >= 0.0):
        raise ValueError(f"eta must be finite and >= 0, got {eta!r}")
    sigma = ddpm.ddim_sigma(eta) if eta != 0.0 else None
    form = _chain_form(ddpm, guided=guidance_scale is not None)

    @torch.no_grad()
    def sample(xT, condition=None):
        engine = _fast_engine(eps_model, ddpm, xT)
        condition = _guided_condition(xT, condition, guidance_scale)
        _need_fused(engine, form)
        if engine is not None:
            nv = _none_value(likelihood, xT) if likelihood is not None else 0.0
            return _run_fast(engine, ddpm, xT, _lib.DDIM, condition, none_value=nv, guidance_scale=guidance_scale, ddim_sigma=sigma, feature_cache=form.feature_cache, tiling=form.tiling)
        kind, step_args = ("ddim", lambda i: ()) if sigma is None else ("ddim_eta", lambda i: (float(sigma[i]),))
        return _run_host(eps_model, ddpm, xT, form, kind, step_args, cond=condition, concat=condition is not None,
                         none=_guided_none(xT, condition, guidance_scale, likelihood), w=guidance_scale)

    return sample
