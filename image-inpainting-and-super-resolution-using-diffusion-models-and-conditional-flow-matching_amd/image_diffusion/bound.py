"""The variational bound (NLL in bits/dim) of a DDPM net on held-out data.  BUILD-DEFINED EXTENSION: the reference trains with the simple loss
(`AD/image_diffusion/loss_functions.py`) and never evaluates the bound; the quantities are those of guided-diffusion's calc_bpd_loop (Ho et al.
2020; Nichol & Dhariwal 2021), the formulas are stated in include/mi355_sampler.h at mi355_ddpm_vlb.

For every step k of the chain, x0 is noised to x_k, the net is evaluated once, and one HIP launch (csrc/vlb.hip) reduces the step's KL - at k = 0
the discretised decoder's NLL - and two diagnostics per image; the prior term closes the sum.  All K steps of a batch run inside ONE library
call, so the function needs an eps_model made by make_eps_model(network, ddpm), as tiling and the feature cache do.  Forward only: nothing here
builds an autograd graph.

bits/dim of a real checkpoint is unmeasured (no trained checkpoint is available offline); what is tested is the arithmetic.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import torch

from .conditioning import Amortized, ClassifierFreeGuidance, Conditioning
from .likelihoods import Likelihood
from .sde_diffusion import DDPM

VARIANCES = ("learned", "fixed_small", "fixed_large")


class VLBResult(NamedTuple):
    total_bpd: torch.Tensor    # [B]     prior_bpd + sum_k vb[:, k]
    prior_bpd: torch.Tensor    # [B]     KL(q(x_K | x0) || N(0, 1))
    vb: torch.Tensor           # [B, K]  step k's term: the KL for k > 0, the decoder's NLL at k = 0
    xstart_mse: torch.Tensor   # [B, K]  mean((x0_hat - x0)^2)
    mse: torch.Tensor          # [B, K]  mean((out - target)^2), target z_k ("eps" chains), x0 ("x0"), sa z_k - sb x0 ("v")


def _refuse(pair: str, why: str):
    raise NotImplementedError(f"get_vlb_fn with {pair}: {why}")


def get_vlb_fn(eps_model: Callable, ddpm: DDPM, conditioning: Optional[Conditioning] = None, likelihood: Optional[Likelihood] = None, *,
               variance: Optional[str] = None, cdf: str = "exact", clip_denoised: bool = True):
    """-> vlb(x0, condition=None, y=None, noise=None, seed=None) -> VLBResult, every field float32 on x0's device.

    variance: "learned" (the net writes eps | v; the range between the posterior variance and beta), "fixed_small" (the posterior variance) or
    "fixed_large" (beta); None: "learned" on a with_learned_variance chain, "fixed_large" on a with_fixed_variance("large") one, "fixed_small"
    otherwise.  The prediction kind is the chain's (DDPM.with_prediction): x0_hat and the mse target follow it (mi355_ddpm_vlb_pred).  cdf: "exact" (erfc) or "tanh"
    (guided-diffusion's approximation, for comparison with published numbers).  Under Amortized conditioning the net sees x_k | condition;
    condition None: x_k | likelihood.none_like.  y: class labels of a class-conditional net.  noise: [K, B, C, H, W] injected draws (draw j
    belongs to step K-1-j), else device Philox at seed (None: torch's initial seed).  A chain view carrying x0 shaping, tiling or a feature cache,
    and a guided conditioning (a guided model's sum is not a bound), raise NotImplementedError naming the pair."""
    from . import sampling

    if cdf not in ("exact", "tanh"):
        raise ValueError(f'cdf must be "exact" or "tanh", got {cdf!r}')
    for attr, pair in (("x0_shaping", "x0_shaping (DDPM.with_x0_shaping)"), ("tiling", "tiling (DDPM.with_tiling)"),
                       ("feature_cache", "feature_cache (DDPM.with_feature_cache)")):
        if getattr(ddpm, attr, None) is not None:
            _refuse(pair, "the bound is defined for the chain's own posterior and whole-frame evaluations; pass the plain chain")
    if isinstance(conditioning, ClassifierFreeGuidance) or getattr(conditioning, "guidance_scale", None) is not None:
        _refuse("guidance_scale (ClassifierFreeGuidance)", "a guided model's sum is not a bound; evaluate the conditional model (Amortized)")
    if variance is None:
        variance = ("learned" if getattr(ddpm, "learned_variance", False) else
                    "fixed_large" if getattr(ddpm, "fixed_variance", "small") == "large" else "fixed_small")
    if variance not in VARIANCES:
        raise ValueError(f"variance must be one of {VARIANCES} or None, got {variance!r}")
    logs = ddpm.vlb_log_variances(variance)   # Ns < 2: ValueError
    learned = variance == "learned"
    amortized = isinstance(conditioning, Amortized)
    if amortized and likelihood is None:
        raise ValueError("Amortized conditioning needs the likelihood (its none_like is what the net sees without a condition)")
    times = torch.tensor([ddpm.time(k) for k in range(ddpm.Ns)], dtype=torch.float32)
    prediction = getattr(ddpm, "prediction", "eps")

    @torch.no_grad()
    def vlb(x0, condition=None, y=None, noise=None, seed=None):
        engine = sampling._fast_engine(eps_model, ddpm, x0)
        if engine is None:
            raise NotImplementedError("the bound runs inside the fused loop: pass an eps_model built by make_eps_model(network, ddpm) for this "
                                      "schedule and device tensors (an arbitrary callable is not evaluated step by step here)")
        if condition is not None and not amortized:
            raise ValueError("a condition needs Amortized conditioning (the net then takes x_k | condition)")
        out_channels = getattr(engine, "out_channels", None)
        if out_channels is not None and out_channels != x0.shape[1] * (2 if learned else 1):
            raise ValueError(f'the net writes {out_channels} channels for data of {x0.shape[1]}: variance "{variance}" needs ' +
                             ("twice the data's channels (eps | v)" if learned else "the data's channels"))
        x = x0.detach().float().contiguous()
        if seed is None:
            seed = int(torch.initial_seed()) & ((1 << 63) - 1)
        nz = None if noise is None else noise.to(x.device, torch.float32).contiguous()
        terms, summary = engine.ddpm_vlb(x, ddpm.host_tables(), logs, learned=learned, times=times,
                                         cond=None if condition is None else condition.float().contiguous(), y=y, noise=nz, seed=seed, cdf=cdf,
                                         clip_denoised=clip_denoised, none_value=sampling._none_value(likelihood, x) if amortized else 0.0,
                                         **({} if prediction == "eps" else {"prediction": prediction}))
        return VLBResult(summary[:, 1], summary[:, 0], terms[:, :, 0], terms[:, :, 1], terms[:, :, 2])

    return vlb
