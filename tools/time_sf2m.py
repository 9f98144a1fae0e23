#!/usr/bin/env python3
"""Cost of the SF2M stochastic sampler on the torchcfm notebooks' workload: two MNIST U-Nets (torchcfm UNetModel(dim=(1, 28, 28),
num_channels=32, num_res_blocks=1): the flow `model` and the `score_model`) at B = 100, torchsde.sdeint(ts=[0, 1], dt=0.01) = 101
Euler-Maruyama steps, timed with device events in one process, the variants interleaved round by round:

  fast      sdeint(SF2MSDE(model, score_model))             one mi355_sf2m_euler_sample call (device Philox noise)
  fast_k10  the same with class-conditional nets (num_classes = 10) and labels arange(10).repeat(10)  (conditional_mnist.ipynb)
  host      sdeint(<the notebook's own SDE class>)          the host-driven loop: sde.f, sde.g and the step op per step
  floor     engine.cfm_euler of each net over the same grid  two forwards per step with the Euler update fused into the last conv

Reports ms per step and the SDE loop's overhead over the floor (two forwards).  Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-inpainting-and-super-resolution-using-diffusion-models-and-conditional-flow-matching_amd"))

import torch  # noqa: E402

from image_diffusion.unet import param_shapes  # noqa: E402
from mi355.synth import randn, synth_state_dict  # noqa: E402
from torchcfm_compat import ClassCondUNetModelWrapper, UNetModelWrapper  # noqa: E402
from torchsde_compat import SF2MSDE, sdeint, step_grid  # noqa: E402


class NotebookSDE(torch.nn.Module):
    """conditional_mnist.ipynb's SDE class as written there."""

    noise_type = "diagonal"
    sde_type = "ito"

    def __init__(self, ode_drift, score, labels=None, reverse=False, sigma=0.1):
        super().__init__()
        self.drift, self.score, self.reverse, self.labels, self.sigma = ode_drift, score, reverse, labels, sigma

    def f(self, t, y):
        y = y.view(-1, 1, 28, 28)
        if self.reverse:
            t = 1 - t
            return -self.drift(t, y, self.labels) + self.score(t, y, self.labels)
        return self.drift(t, y, self.labels).flatten(start_dim=1) + self.score(t, y, self.labels).flatten(start_dim=1)

    def g(self, t, y):
        return torch.ones_like(y) * self.sigma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sf2m.py needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")

    def pair(cls, seed, **kw):
        nets = []
        for s in (seed, seed + 1):
            m = cls(dim=(1, 28, 28), num_channels=32, num_res_blocks=1, precision=a.precision, **kw)
            m.load_state_dict(synth_state_dict(param_shapes(m), s))
            nets.append(m.to(dev))
        return nets

    m, sm = pair(UNetModelWrapper, 5101)
    mk, smk = pair(ClassCondUNetModelWrapper, 5201, num_classes=10, class_cond=True)
    B = a.batch
    y0 = randn(5301, B, 784).to(dev)
    labels = torch.arange(10, device=dev).repeat((B + 9) // 10)[:B]
    ts = torch.linspace(0, 1, 2, device=dev)
    grid, _ = step_grid(ts, 0.01)
    n = len(grid) - 1

    def floor():
        x = y0.view(B, 1, 28, 28).clone()
        m.engine(dev).cfm_euler(x, grid)
        sm.engine(dev).cfm_euler(x, grid)
        return x

    variants = {
        "fast": lambda: sdeint(SF2MSDE(m, sm, sigma=0.1), y0, ts, dt=0.01),
        "fast_k10": lambda: sdeint(SF2MSDE(mk, smk, labels=labels, sigma=0.1), y0, ts, dt=0.01),
        "host": lambda: sdeint(NotebookSDE(m, sm, sigma=0.1), y0, ts, dt=0.01),
        "floor": floor,
    }

    def run(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = variants[name]()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n, out

    for name in variants:   # warm-up: code objects, workspaces, engines, every shape of the timed window
        run(name)
        run(name)
    ms = {k: [] for k in variants}
    finals = {}
    for _ in range(a.rounds):
        for name in variants:
            t, out = run(name)
            ms[name].append(t)
            finals[name] = out
    for e in (m, sm, mk, smk):
        e.engine(dev).check()
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {
        "config": "mnist nc32 nrb1 B=%d %s, %d steps (ts=[0,1], dt=0.01), sigma 0.1" % (B, a.precision, n),
        "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
        "ms_per_step_spread": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "sde_over_two_forwards_pct": round(100.0 * (med["fast"] / med["floor"] - 1.0), 2),
        "sde_k10_over_two_forwards_pct": round(100.0 * (med["fast_k10"] / med["floor"] - 1.0), 2),
        "host_over_fast": round(med["host"] / med["fast"], 3),
        "finite": all(bool(torch.isfinite(v).all()) for v in finals.values()),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
