"""CPU restatement of the training-free flow in-painting / super-resolution sampler (mi355_cfm_recon_sample) and of the low-resolution
consistency seed (mi355_lowres_seed), under torch.autograd.  There is no reference counterpart (the reference has replacement and
reconstruction guidance for diffusion only), so this module is the expectation the GPU tests compare against, like
tests/test_classcond_cpu.classcond_forward for class labels.

Conventions: t runs from 0 (noise) to 1 (data), the net's output is the velocity v(t, x), the data estimate is x1_hat = x + (1 - t) v.
"""
from typing import Callable, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import ddpm_ref, unet_ref


# ---- the down-sampling operator and its adjoint ---------------------------------------------------------------------------------

def lowres_D(x: torch.Tensor, size) -> torch.Tensor:
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)


def axis_taps(n_out: int, n_in: int):
    """The two source taps of every output index along one axis, in ATen's fp32 arithmetic (area_pixel_compute_source_index, align_corners
    False): (i0, i1 long [n_out], l0, l1 float32 [n_out])."""
    scale = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
    o = torch.arange(n_out, dtype=torch.float32)
    f = (scale * (o + 0.5) - 0.5).clamp_min(0.0)
    i0 = f.floor().long()
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = (f - i0.float()).clamp(0.0, 1.0)
    return i0, i1, 1.0 - l1, l1


def axis_gather_weights(n_out: int, n_in: int, dtype):
    """Gather form of the adjoint along one axis, for n_in % n_out == 0: source index Y receives from output index Y // s only, with weight
    l0 if Y is that output's first tap, l1 if it is its second (their sum if both), else 0.  -> (low index long [n_in], weight [n_in])."""
    assert n_in % n_out == 0
    i0, i1, l0, l1 = axis_taps(n_out, n_in)
    Y = torch.arange(n_in)
    low = Y // (n_in // n_out)
    w = (Y == i0[low]).to(dtype) * l0[low].to(dtype) + (Y == i1[low]).to(dtype) * l1[low].to(dtype)
    return low, w


def lowres_DT_gather(r: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """D^T r for r [B, C, h, w] with H % h == 0 and W % w == 0, in r's dtype: [B, C, H, W]."""
    ly, wy = axis_gather_weights(r.shape[2], H, r.dtype)
    lx, wx = axis_gather_weights(r.shape[3], W, r.dtype)
    return (wy[:, None] * wx[None, :]) * r[:, :, ly][:, :, :, lx]


# ---- per-sample constraint losses at the data estimate --------------------------------------------------------------------------

def constraint_loss(x1: torch.Tensor, y: torch.Tensor, mode: int, pad_value: float = -2.0) -> torch.Tensor:
    """[B]: mode 0 Painting.loss, 1 HyperResolution.loss (per sample), 2 mean((D(x1) - y)^2) with D the bilinear reduction to y's size."""
    if mode == 0:
        return ddpm_ref.painting_loss(x1, y, pad_value)
    if mode == 1:
        return ddpm_ref.hyperres_loss(x1, y)
    return ((lowres_D(x1, y.shape[2:]) - y) ** 2).mean(dim=(1, 2, 3))


def flow_guidance_grad(forward: Callable, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor, mode: int, pad_value: float = -2.0):
    """-> (v, grad_x sum_n loss_n(clip(x + (1 - t) v(t, x), -1, 1), y), per-sample losses), all detached; t a 0-dim fp32 tensor."""
    omt = torch.tensor(1.0, dtype=torch.float32) - t
    with torch.enable_grad():
        xr = x.detach().clone().requires_grad_()
        v = forward(xr, t.expand(x.shape[0]))
        losses = constraint_loss(torch.clip(xr + omt * v, -1, 1), y, mode, pad_value)
        (g,) = torch.autograd.grad(losses.sum(), xr)
    return v.detach(), g, losses.detach()


def flow_recon_ref(sd, cfg, x0: torch.Tensor, t_span: Sequence[float], y: Optional[torch.Tensor], mode: int, scales: Optional[Sequence[float]] = None,
                   replace: Optional[str] = None, final_paste: bool = False, pad_value: float = -2.0, noise: Optional[torch.Tensor] = None,
                   forward: Optional[Callable] = None):
    """The sampler, step by step in fp32 on the CPU.  forward(x, t[B]) defaults to unet_ref.unet_forward_diff(sd, cfg, x, t) (pass a closure for
    class labels).  replace: None, "coupled" (z = x0) or "fresh" (z = noise[k]).  The loss is summed over samples: one gradient per step.
    -> dict(x, traj [n_t, ...], losses [n_steps, B] (NaN where a step was not guided))."""
    if forward is None:
        forward = lambda x, t: unet_ref.unet_forward_diff(sd, cfg, x, t)   # noqa: E731
    ts = torch.tensor([float(v) for v in t_span], dtype=torch.float32)
    one = torch.tensor(1.0, dtype=torch.float32)
    x = x0.detach().clone().float()
    n_steps = len(ts) - 1
    traj = [x.clone()]
    losses = torch.full((n_steps, x.shape[0]), float("nan"))

    def paste(x, k):
        z = x0 if replace == "coupled" else noise[k]
        return torch.where(y == pad_value, x, ts[k] * y + (one - ts[k]) * z)

    for k in range(n_steps):
        t, dt = ts[k], ts[k + 1] - ts[k]
        if replace is not None:
            x = paste(x, k)
        s = 0.0 if scales is None else float(scales[k])
        if s != 0.0:
            v, g, losses[k] = flow_guidance_grad(forward, x, t, y, mode, pad_value)
            c = dt * torch.tensor(s, dtype=torch.float32)
            x = x + (dt * v - c * g)
        else:
            with torch.no_grad():
                x = x + dt * forward(x, t.expand(x.shape[0]))
        traj.append(x.clone())
    if final_paste:
        x = paste(x, n_steps)
        traj[-1] = x.clone()
    return dict(x=x, traj=torch.stack(traj), losses=losses)


# ---- mi355_lowres_seed in fp64, from the fp32 inputs and the fp32 tap weights ---------------------------------------------------

def lowres_seed_ref64(x: torch.Tensor, eps: torch.Tensor, y_low: torch.Tensor, c_recip: float, c_recipm1: float):
    """What the seed computes, every operation in fp64 on the fp32 operands (the coefficients rounded to fp32 first), together with the
    magnitudes the rounding bounds are made of.  -> dict(pre, resid, loss, g_eps, g_x, M_resid, M_loss, M_g): M_resid the sum of the absolute
    values of the terms of a residual, M_loss the per-sample mean of M_resid^2, M_g the magnitude of g = k w resid (k = 2 / per in fp32).
    NaN propagates as in the kernel: through the residual and the products, and g is 0 wherever pre is NaN or outside [-1, 1]."""
    B, C, H, W = x.shape
    h, w = y_low.shape[2:]
    cr = float(torch.tensor(c_recip, dtype=torch.float32))
    cm = float(torch.tensor(c_recipm1, dtype=torch.float32))
    xd, ed, yd = x.double(), eps.double(), y_low.double()
    pre = cr * xd - cm * ed
    mag = (cr * xd).abs() + (cm * ed).abs()
    x0 = torch.where(pre < -1, -1.0, torch.where(pre > 1, 1.0, pre))            # NaN passes (both comparisons false)
    yi0, yi1, yl0, yl1 = axis_taps(h, H)
    xi0, xi1, xl0, xl1 = axis_taps(w, W)

    def D(v):
        r0 = xl0.double() * v[:, :, yi0][:, :, :, xi0] + xl1.double() * v[:, :, yi0][:, :, :, xi1]
        r1 = xl0.double() * v[:, :, yi1][:, :, :, xi0] + xl1.double() * v[:, :, yi1][:, :, :, xi1]
        return yl0.double()[:, None] * r0 + yl1.double()[:, None] * r1

    resid = D(x0) - yd
    M_resid = D(torch.nan_to_num(mag, nan=0.0)) + yd.abs()
    per = C * h * w
    loss = (resid * resid).mean(dim=(1, 2, 3))
    M_loss = (M_resid * M_resid).mean(dim=(1, 2, 3))
    k = float(torch.tensor(2.0, dtype=torch.float32) / torch.tensor(float(per), dtype=torch.float32))
    ly, wy = axis_gather_weights(h, H, torch.float64)
    lx, wx = axis_gather_weights(w, W, torch.float64)
    wgt = wy[:, None] * wx[None, :]
    g = k * (wgt * resid[:, :, ly][:, :, :, lx])
    M_g = k * (wgt * M_resid[:, :, ly][:, :, :, lx])
    inside = (pre >= -1) & (pre <= 1)
    g = torch.where(inside, g, 0.0)
    M_g = torch.where(inside, M_g, 0.0)
    return dict(pre=pre, resid=resid, loss=loss, g_eps=-cm * g, g_x=cr * g, M_resid=M_resid, M_loss=M_loss, M_g_eps=abs(cm) * M_g,
                M_g_x=abs(cr) * M_g)


# ---- DDPM ReconstructionGuidance with the low-resolution likelihood -------------------------------------------------------------

def ddpm_lowres_guidance_ref(eps_model, Ns: int, xT: torch.Tensor, y_low: torch.Tensor, noise, *, gamma: float, start_fraction: float = 1.0):
    """oracle.ddpm_ref.recon_guidance_sample's loop, rule "before", no corrector, with the constraint mean((D(x0_hat) - y_low)^2): built
    from ddpm_ref's tables and step functions, the gradient from torch.autograd."""
    ddpm = ddpm_ref.DDPMRef(Ns)
    alphas = ddpm.t["alphas"]
    x0_model = ddpm_ref._x0_model(eps_model, ddpm, False, None)
    xi = xT.clone()
    for i in reversed(range(Ns)):
        if i < int(Ns * start_fraction):
            with torch.enable_grad():
                xr = xi.detach().clone().requires_grad_()
                (x_grad,) = torch.autograd.grad(constraint_loss(x0_model(xr, i), y_low, 2).sum(), xr)
            xi = xi + -(gamma * alphas[i] * (1 - alphas[i])) * x_grad
        with torch.no_grad():
            xi = ddpm_ref._ancestral(ddpm, x0_model(xi, i), xi, i, noise)
    return torch.clip(xi.detach(), -1, 1)
