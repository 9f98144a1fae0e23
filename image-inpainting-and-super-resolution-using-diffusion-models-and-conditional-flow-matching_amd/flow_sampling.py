"""Training-free in-painting and super-resolution with an UNCONDITIONAL flow-matching net: the flow counterpart of
`image_diffusion.sampling.get_conditional_sample_fn`.

    get_flow_conditional_sample_fn(model, conditioning, likelihood, t_span) -> sample(x0, condition)

model: a `UNetModelWrapper`, `ClassCondUNetModelWrapper` or `UNetModel` (anything with the packed HIP engine); conditioning: a `FlowReplacement`
or `FlowReconstructionGuidance`; likelihood: `InPainting` / `OutPainting` (replacement and guidance), `HyperResolution` or `LowResolution`
(guidance); t_span: the Euler time grid from 0 (noise) to 1 (data).  x0 is the noise the flow starts from, condition what `likelihood.sample`
made of the image.  The first int(n_steps * start_fraction) steps are one `UNetEngine.cfm_recon` call (mi355_cfm_recon_sample: paste, forward,
seed, U-Net VJP and the fused update of every step inside the library), the remaining ones the plain engine's `cfm_euler`.  The reference has
these two methods for diffusion only; the convention, rounding order and refusals are in DESIGN.md section 5.10.
"""
from __future__ import annotations

from typing import Sequence

import torch

from image_diffusion.conditioning import Conditioning, FlowReconstructionGuidance, FlowReplacement, flow_split_index
from image_diffusion.likelihoods import Likelihood
from mi355._lib import MI355BackendError


def _likelihood_mode(likelihood: Likelihood):
    """-> (mode of mi355_cfm_recon_sample, pad value)"""
    if hasattr(likelihood, "pad_value"):
        return 0, float(likelihood.pad_value)
    name = type(likelihood).__name__
    if name == "HyperResolution":
        return 1, 0.0
    if name == "LowResolution":
        return 2, 0.0
    raise NotImplementedError(f"no constraint gradient for likelihood {name}")


def get_flow_conditional_sample_fn(model, conditioning: Conditioning, likelihood: Likelihood, t_span: Sequence[float]):
    """sample(x0, condition, y=None, noise=None, seed=None) -> the image batch, fp32, not clipped (as the CFM samplers return it).
    y: class labels [B] of a class-conditional model.  noise / seed: the draws of a "fresh" replacement ([n_draws, B, C, H, W] injected, or the
    Philox key; seed None: drawn from torch's default generator)."""
    if not hasattr(model, "engine"):
        raise NotImplementedError(
            "the flow samplers run inside the HIP library and differentiate through the network: pass a UNetModelWrapper, "
            "ClassCondUNetModelWrapper or UNetModel (an arbitrary callable has no engine and no backward pass on the HIP backend)")
    ts = [float(v) for v in t_span]
    n_steps = len(ts) - 1
    if n_steps < 1:
        raise ValueError("t_span needs at least two times (one step)")
    mode, pad = _likelihood_mode(likelihood)
    if isinstance(conditioning, FlowReconstructionGuidance):
        guided, replace = True, conditioning.replace
    elif isinstance(conditioning, FlowReplacement):
        guided, replace = False, conditioning.noise
    else:
        raise NotImplementedError(f"no flow sampler for conditioning type {type(conditioning).__name__}")
    if replace is not None and mode != 0:
        raise ValueError("replacement pastes the known pixels of a painting condition: it needs an InPainting / OutPainting likelihood")
    n_g = flow_split_index(n_steps, conditioning.start_fraction)
    scales = conditioning.scales(ts[:n_g]) if guided else None

    @torch.no_grad()
    def sample(x0, condition, y=None, noise=None, seed=None):
        if not x0.is_cuda:
            raise MI355BackendError("the flow samplers need device tensors (no CPU fallback)")
        x = x0.detach().clone().float().contiguous()
        condition = condition.to(x.device).float().contiguous()
        eng = model.engine(x.device)
        if n_g > 0:
            geng = model.engine(x.device, differentiable=True) if guided else eng
            geng.cfm_recon(x, ts[:n_g + 1], condition, mode, scales=scales, replace=replace, final_paste=replace is not None and n_g == n_steps,
                           pad_value=pad, noise=noise, seed=seed, y_labels=y)
        if n_g < n_steps:
            eng.cfm_euler(x, ts[n_g:], y=y)
        return x

    return sample
