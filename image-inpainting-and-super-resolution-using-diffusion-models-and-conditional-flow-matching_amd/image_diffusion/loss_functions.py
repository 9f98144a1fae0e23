"""Counterpart of `AD/image_diffusion/loss_functions.py:13-62` (get_loss_function), forward only: the value of the denoising loss
mean_b mean_chw (eps_model(x_i, i) - noise)^2 on the HIP path.  Training stays out of scope: nothing here builds an autograd graph, the returned
loss is a number to report (a validation loss), not something to call backward() on.

The reference's three draws keep their defaults and can each be overridden by a keyword of loss(x, i=None, noise=None, use_condition=None):
    i              the per-image step, torch.randint(0, Ns, (b,))                                  loss_functions.py:24, 54
    noise          torch.randn_like(x)                         (ddpm.q_sample)                     sde_diffusion.py:239-244
    use_condition  the p_cond coin torch.rand(()) < conditioning.p_cond   (Amortized only)         loss_functions.py:47-50
drawn in the reference's order (the coin, the steps, the noise).  The net runs once at per-image times through the existing forward; the noising
is mi355_lincomb_per_sample, the reduction mi355_mse_per_sample.
"""
from __future__ import annotations

import torch

from mi355.ops import default_ops

from .conditioning import Amortized, Conditioning
from .likelihoods import Likelihood
from .sampling import make_eps_model
from .sde_diffusion import DDPM, Network


def _steps(ddpm, x, i):
    b = x.shape[0]
    if i is None:
        return torch.randint(0, ddpm.Ns, (b,), device=x.device).long()
    i = torch.as_tensor(i, device=x.device).long()
    if tuple(i.shape) != (b,):
        raise ValueError(f"i must have shape ({b},), got {tuple(i.shape)}")
    if b and (int(i.min()) < 0 or int(i.max()) >= ddpm.Ns):
        raise ValueError(f"i must lie in [0, {ddpm.Ns})")
    return i


def _noised(ddpm, x, i, noise):
    """ddpm.q_sample with the draw given or left to torch.randn_like -> (x_i, noise), both float32 and contiguous."""
    x = x.float().contiguous()
    if noise is None:
        xi, noise = ddpm.q_sample(x, i)
        return xi, noise.float().contiguous()
    if noise.shape != x.shape:
        raise ValueError(f"noise must have x's shape {tuple(x.shape)}, got {tuple(noise.shape)}")
    noise = noise.to(x.device, torch.float32).contiguous()
    return ddpm._lin(x, ddpm._coef(ddpm.sqrt_alphas_cumprod, i, x), noise, ddpm._coef(ddpm.sqrt_one_minus_alphas_cumprod, i, x)), noise


def _mean_mse(noise_hat, noise):
    noise_hat = noise_hat.float().contiguous()
    if noise_hat.shape != noise.shape:
        raise ValueError(f"the net writes {tuple(noise_hat.shape)} for noise of {tuple(noise.shape)}: the simple loss compares eps with the draw "
                         "(a learned-variance net's bound is image_diffusion.bound.get_vlb_fn)")
    return default_ops.mse_per_sample(noise_hat, noise).mean()


def get_loss_function(network: Network, ddpm: DDPM, conditioning: Conditioning, likelihood: Likelihood):
    """-> (loss, eps_model).  Generic conditioning (loss_functions.py:13-33): loss(x) = mean over the batch of the per-image mean squared error
    of eps_model(x_i, i) against the noise.  Amortized (loss_functions.py:36-62): the net sees x_i | condition, the condition being
    likelihood.sample(x) with probability p_cond and likelihood.none_like(x) otherwise.  eps_model is make_eps_model(network, ddpm), the model
    the samplers take.  Builds no autograd graph."""
    eps_model = make_eps_model(network, ddpm)
    if isinstance(conditioning, Amortized):   # dispatch on the type, as image_diffusion.sampling does (a ClassifierFreeGuidance is one)
        @torch.no_grad()
        def loss(x, i=None, noise=None, use_condition=None):
            if use_condition is None:
                use_condition = bool(torch.rand(()) < conditioning.p_cond)
            condition = likelihood.sample(x) if use_condition else likelihood.none_like(x)
            i = _steps(ddpm, x, i)
            xi, noise = _noised(ddpm, x, i, noise)
            xi_condition = torch.cat((xi, condition.to(xi.device, torch.float32)), dim=-3).contiguous()
            return _mean_mse(eps_model(xi_condition, i), noise)

        return loss, eps_model

    @torch.no_grad()
    def loss(x, i=None, noise=None, use_condition=None):
        if use_condition is not None:
            raise ValueError("use_condition belongs to Amortized conditioning (the p_cond coin); this loss takes no condition")
        i = _steps(ddpm, x, i)
        xi, noise = _noised(ddpm, x, i, noise)
        return _mean_mse(eps_model(xi, i), noise)

    return loss, eps_model
