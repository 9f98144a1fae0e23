"""Stand-in for the un-vendored `torchsde` as the torchcfm notebooks call it (mnist_example.ipynb and conditional_mnist.ipynb, third section,
"SF2M"): an `SDE` module whose drift is model + score_model and whose diffusion is the constant sigma, integrated by

    torchsde.sdeint(sde, y0 [B, 784], ts=torch.linspace(0, 1, 2), dt=0.01)

torchsde is not in the reference and not on this build's machines; what is restated here is its fixed-step loop and Euler step (versions
unpinned):
  - the step grid: curr_t = ts[0]; for each output time, while curr_t < out_t: next_t = min(curr_t + dt, ts[-1]), all on fp32 tensors, so the
    boundaries accumulate in fp32 (ts = [0, 1], dt = 0.01: 101 steps, the last one 6.5565e-7 long: the notebook runs 202 U-Net forwards);
  - an output time inside a step is the linear interpolation y_k + (t - t_k) / (t_{k+1} - t_k) * (y_{k+1} - y_k) of the two states around it
    (the end points themselves when t equals one of them);
  - the Euler(-Maruyama) step y_{k+1} = y_k + f(t_k, y_k) * dt + g(t_k, y_k) * dW_k.
torchsde picks a stochastic Runge-Kutta scheme (method "srk") by default for diagonal Ito noise (recalled, not checked: torchsde is not here).
Because g is constant in these notebooks, Euler-Maruyama and Milstein coincide, but SRK differs: this build runs Euler-Maruyama for
method=None and "euler", and parity with the notebook's default solver is unpinned, like dopri5's.

Brownian increments: bm=None draws them on the device (Philox, keyed by a seed taken from torch's default generator, so torch.manual_seed
reproduces a run); a `bm` with torchsde's interface bm(ta, tb) -> W(tb) - W(ta) is evaluated once per step and its increments are injected.

SF2MSDE is the notebooks' SDE class.  sdeint(SF2MSDE of two engine-backed torchcfm_compat models, y0 on the device) is ONE library call
(mi355_sf2m_euler_sample: both forwards and the fused update of every step); any other SDE module - the notebook's own class included -
takes the host-driven loop: sde.f, then sde.g, then the HIP Euler-Maruyama step op.  There is no CPU path.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch

from mi355._lib import MI355BackendError
from mi355.ops import default_ops
from torchcfm_compat import ClassCondUNetModelWrapper, UNetModelWrapper


class SF2MSDE(torch.nn.Module):
    """The notebooks' `SDE(ode_drift, score, labels=None, reverse=False, sigma=0.1)`: diagonal Ito noise, drift
    f(t, y) = ode_drift(t, y, labels) + score(t, y, labels) (reverse: both at 1 - t, -ode_drift + score), diffusion g = sigma.
    y may have any shape whose trailing size is C*H*W of the nets (the notebooks pass [B, 784]); f and g return y's shape.  The notebook's
    reverse branch returns [B, 1, 28, 28] for a flattened y, which cannot be added to it; here both directions return y's shape."""

    noise_type = "diagonal"
    sde_type = "ito"

    def __init__(self, ode_drift, score, labels=None, reverse=False, sigma=0.1):
        super().__init__()
        self.drift = ode_drift
        self.score = score
        self.reverse = reverse
        self.labels = labels
        self.sigma = sigma

    def _image_shape(self):
        m = self.drift
        if hasattr(m, "in_channels") and hasattr(m, "image_size"):
            return (int(m.in_channels), int(m.image_size), int(m.image_size))
        return (1, 28, 28)   # the notebooks' MNIST view for a model that does not say

    def _call(self, net, t, y):
        return net(t, y) if self.labels is None else net(t, y, self.labels)

    def f(self, t, y):
        yi = y.reshape((-1,) + self._image_shape())
        if self.reverse:
            t = 1 - t
            return (-self._call(self.drift, t, yi) + self._call(self.score, t, yi)).reshape(y.shape)
        return (self._call(self.drift, t, yi) + self._call(self.score, t, yi)).reshape(y.shape)

    def g(self, t, y):
        return torch.ones_like(y) * self.sigma


def step_grid(ts, dt) -> Tuple[List[float], List[Tuple[int, float]]]:
    """torchsde's fixed-step grid over ts with step dt -> (boundaries t_0 .. t_n as fp32 values, [(step k, weight w)] per output time):
    output j is y_k + w * (y_{k+1} - y_k).  Computed on fp32 CPU tensors exactly as torchsde steps its `curr_t` tensor."""
    ts = torch.as_tensor(ts).detach().to("cpu", torch.float32).reshape(-1)
    if ts.numel() < 2 or not bool((ts[1:] > ts[:-1]).all()):
        raise ValueError("ts must hold at least two strictly increasing times")
    if not float(dt) > 0:
        raise ValueError("dt must be positive")
    curr_t = prev_t = ts[0]
    grid = [float(curr_t)]
    outs = [(0, 0.0)]
    for out_t in ts[1:]:
        while curr_t < out_t:
            next_t = min(curr_t + dt, ts[-1])
            prev_t, curr_t = curr_t, next_t
            grid.append(float(curr_t))
        k = len(grid) - 2
        if out_t == prev_t:
            w = 0.0
        elif out_t == curr_t:
            w = 1.0
        else:
            w = float((out_t - prev_t) / (curr_t - prev_t))
        outs.append((k, w))
    return grid, outs


def _engine_backed(m) -> bool:
    return type(m) in (UNetModelWrapper, ClassCondUNetModelWrapper)


def _fast_path(sde, y0) -> bool:
    if type(sde) is not SF2MSDE or not (_engine_backed(sde.drift) and _engine_backed(sde.score)):
        return False
    d, s = sde.drift, sde.score
    return (d.num_classes == s.num_classes and d.in_channels == d.out_channels == s.in_channels == s.out_channels
            and d.image_size == s.image_size and y0.numel() % (d.in_channels * d.image_size ** 2) == 0
            and isinstance(sde.sigma, (int, float)))


@torch.no_grad()
def sdeint(sde, y0, ts, bm=None, method=None, dt=1e-3, adaptive=False, rtol=1e-5, atol=1e-4, dt_min=1e-5, options=None, names=None,
           logqp=False, extra=False, extra_solver_state=None, **unused_kwargs):
    """torchsde.sdeint restated for fixed-step Euler-Maruyama on the MI355X -> Tensor [len(ts), *y0.shape] (the states at ts)."""
    if method not in (None, "euler"):
        raise NotImplementedError(f"method={method!r}: this build integrates with Euler-Maruyama only (method=None or 'euler')")
    if adaptive:
        raise NotImplementedError("adaptive=True: this build has fixed-step Euler-Maruyama only")
    if logqp:
        raise NotImplementedError("logqp=True is not built")
    if extra:
        raise NotImplementedError("extra=True is not built (Euler-Maruyama has no extra solver state)")
    sde_type, noise_type = getattr(sde, "sde_type", None), getattr(sde, "noise_type", None)
    if sde_type != "ito":
        raise NotImplementedError(f"sde_type={sde_type!r}: only 'ito' SDEs are built")
    if noise_type != "diagonal":
        raise NotImplementedError(f"noise_type={noise_type!r}: only 'diagonal' noise is built")
    if not isinstance(y0, torch.Tensor) or not y0.is_cuda:
        raise MI355BackendError(f"y0 is on {getattr(y0, 'device', type(y0))}: sdeint needs an MI355X device tensor (no CPU fallback)")
    if names:
        raise NotImplementedError("names=: the SDE module's drift and diffusion are its methods f and g here")
    f_fn, g_fn = sde.f, sde.g
    grid, outs = step_grid(ts, dt)
    n = len(grid) - 1
    dev = y0.device
    y = y0.detach().to(torch.float32).contiguous().clone()
    dW = None
    if bm is not None:
        tg = torch.tensor(grid, dtype=torch.float32, device=dev)
        dW = torch.stack([torch.as_tensor(bm(tg[k], tg[k + 1]), device=dev).to(torch.float32).reshape(y.shape) for k in range(n)]).contiguous()
    seed = None if dW is not None else int(torch.randint(0, 2 ** 62, (1,)).item())

    if _fast_path(sde, y0):
        d, s = sde.drift, sde.score
        shape = (-1, d.in_channels, d.image_size, d.image_size)
        x = y.reshape(shape)
        lab = sde.labels if d.num_classes is not None else None
        if d.num_classes is not None and lab is None:
            raise ValueError("y (class labels) is required: the SDE's models were built with class_cond=True and num_classes="
                             f"{d.num_classes}")
        if lab is not None:
            lab = torch.as_tensor(lab, device=dev)
        _, traj = d.engine(dev).sf2m_euler(s.engine(dev), x, grid, float(sde.sigma), bool(sde.reverse), y=lab,
                                           dW=dW.reshape((n,) + tuple(x.shape)) if dW is not None else None, seed=seed, outputs=outs)
        return traj.reshape((len(outs),) + tuple(y0.shape))

    # host-driven: sde.f, sde.g, then the HIP Euler-Maruyama launch (which also writes the step's output time)
    traj = torch.empty((len(outs),) + tuple(y.shape), device=dev, dtype=torch.float32)
    n_al = (y.numel() + 3) // 4 * 4
    tdev = torch.tensor(grid, dtype=torch.float32, device=dev)
    for k in range(n):
        here = [j for j, (kk, _) in enumerate(outs) if kk == k]
        for j in here:
            if outs[j][1] == 0.0:
                traj[j].copy_(y)
        interp = [j for j in here if outs[j][1] != 0.0]
        f = f_fn(tdev[k], y)
        g = g_fn(tdev[k], y)
        f = f.to(torch.float32).contiguous()
        g = g.to(torch.float32).contiguous() if isinstance(g, torch.Tensor) else float(g)
        dw = dW[k] if dW is not None else None
        ph = None if dW is not None else (seed, k * n_al)
        dt_k = float(np.float32(grid[k + 1]) - np.float32(grid[k]))   # fp32, as torchsde's t1 - t0 (and the library's loop)
        for j in interp[1:]:   # several output times inside one step: the same update again on a copy of y_k
            default_ops.sde_euler_step_(y.clone(), f, dt_k, g, dW=dw, philox=ph, out=traj[j], w=outs[j][1])
        default_ops.sde_euler_step_(y, f, dt_k, g, dW=dw, philox=ph, out=traj[interp[0]] if interp else None,
                                    w=outs[interp[0]][1] if interp else 0.0)
    return traj.reshape((len(outs),) + tuple(y0.shape))
