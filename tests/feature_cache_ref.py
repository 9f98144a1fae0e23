"""Restatement of feature reuse across sampler steps (DeepCache: Ma, Fang, Wang, CVPR 2024) on the oracle U-Net (TEST ORACLE; no reference
counterpart).  Built from oracle.unet_ref's build_plan, _run_layers, timestep_embedding and group_norm32, independently of csrc / mi355.

With input_blocks[0..n-1] and output_blocks[0..n-1] of UNetModel, branch k (1 <= k <= n-1) keeps the k outermost block pairs.  The cached
feature F of branch k is h just before torch.cat([h, hs.pop()]) of output_blocks[n-k].  A shallow evaluation computes the embedding of its own
t (and labels), runs input_blocks[0..k-1] on its own x, takes F from the most recent full evaluation, and runs output_blocks[n-k..n-1] and out.
The network runs in fp32 (as the oracle does); the sampler loops around it run in fp64 (the step arithmetic of oracle.cfm_ref and
tests/ddpm_respace_ref.py).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import unet_ref


def n_blocks(cfg) -> int:
    return len(unet_ref.build_plan(cfg)[0])


def _emb(sd, cfg, t, y=None):
    emb = F.linear(unet_ref.timestep_embedding(t, cfg.model_channels), sd["time_embed.0.weight"], sd["time_embed.0.bias"])
    emb = F.linear(F.silu(emb), sd["time_embed.2.weight"], sd["time_embed.2.bias"])
    return emb if y is None else emb + sd["label_emb.weight"][y.long()]


def _out(sd, h):
    return unet_ref._conv(sd, "out.2", F.silu(unet_ref.group_norm32(h, sd["out.0.weight"], sd["out.0.bias"])))


@torch.no_grad()
def full_with_feature(sd, cfg, x, t, k, y=None):
    """UNetModel.forward(x, t[, y]) -> (output, the cached feature of branch k)."""
    input_blocks, middle, output_blocks, _ = unet_ref.build_plan(cfg)
    n = len(input_blocks)
    assert len(output_blocks) == n and 1 <= k <= n - 1, (n, k)
    emb = _emb(sd, cfg, t, y)
    hs, h, feat = [], x.float(), None
    for i, layers in enumerate(input_blocks):
        h = unet_ref._run_layers(sd, cfg, f"input_blocks.{i}", layers, h, emb)
        hs.append(h)
    h = unet_ref._run_layers(sd, cfg, "middle_block", middle, h, emb)
    for i, layers in enumerate(output_blocks):
        if i == n - k:
            feat = h.clone()
        h = unet_ref._run_layers(sd, cfg, f"output_blocks.{i}", layers, torch.cat([h, hs.pop()], dim=1), emb)
    return _out(sd, h), feat


@torch.no_grad()
def shallow(sd, cfg, x, t, k, feat, y=None):
    """The shallow evaluation of branch k at (x, t[, y]) on the cached feature `feat`."""
    input_blocks, _, output_blocks, _ = unet_ref.build_plan(cfg)
    n = len(input_blocks)
    assert 1 <= k <= n - 1, (n, k)
    emb = _emb(sd, cfg, t, y)
    hs, h = [], x.float()
    for i in range(k):
        h = unet_ref._run_layers(sd, cfg, f"input_blocks.{i}", input_blocks[i], h, emb)
        hs.append(h)
    h = feat.float()
    for i in range(n - k, n):
        h = unet_ref._run_layers(sd, cfg, f"output_blocks.{i}", output_blocks[i], torch.cat([h, hs.pop()], dim=1), emb)
    assert not hs
    return _out(sd, h)


def interval_schedule(n_evals: int, interval: int):
    """DeepCache's uniform 1:N schedule."""
    return [e % interval == 0 for e in range(n_evals)]


def drift(cur: torch.Tensor, prev: torch.Tensor) -> torch.Tensor:
    """Per image: ||cur - prev||^2 / ||prev||^2 in fp64, over everything but the batch dimension."""
    c, p = cur.double().flatten(1), prev.double().flatten(1)
    return ((c - p) ** 2).sum(1) / (p ** 2).sum(1)


class CachedNet:
    """The network under a cache schedule: call e (in call order) is full iff full[e]; a shallow call reuses the last full call's feature.
    drifts[e] = drift(F_e, F_prev) per image for every full call after the first, -1 elsewhere."""

    def __init__(self, sd, cfg, k, full):
        self.sd, self.cfg, self.k, self.full = sd, cfg, k, [bool(f) for f in full]
        assert self.full and self.full[0]
        self.e, self.feat, self.drifts = 0, None, []

    def __call__(self, x, t, y=None):
        assert self.e < len(self.full), "more evaluations than the schedule has entries"
        if self.full[self.e]:
            out, feat = full_with_feature(self.sd, self.cfg, x, t, self.k, y)
            self.drifts.append(torch.full((x.shape[0],), -1.0, dtype=torch.float64) if self.feat is None else drift(feat, self.feat))
            self.feat = feat
        else:
            out = shallow(self.sd, self.cfg, x, t, self.k, self.feat, y)
            self.drifts.append(torch.full((x.shape[0],), -1.0, dtype=torch.float64))
        self.e += 1
        return out


def cached_euler(sd, cfg, x0, t_span, k, full, y=None, cond=None):
    """oracle.cfm_ref.euler_trajectory in fp64 around the fp32 network under the schedule: x_{j+1} = x_j + (t_{j+1} - t_j) net_j(t_j, x_j).
    t_span: fp32 values (the differences are taken in fp32, as the sampler takes them).  -> (all len(t_span) states [n_t, B, C, H, W] fp64,
    the drift rows [n_t - 1, B])."""
    net = CachedNet(sd, cfg, k, full)
    ts = torch.as_tensor(t_span, dtype=torch.float32)
    assert len(full) == len(ts) - 1
    x = x0.double()
    xs = [x]
    for j in range(len(ts) - 1):
        xin = x.float() if cond is None else torch.cat((x.float(), cond.float()), dim=1)
        v = net(xin, torch.full((x.shape[0],), float(ts[j]), dtype=torch.float32), y)
        x = x + float(ts[j + 1] - ts[j]) * v.double()
        xs.append(x)
    return torch.stack(xs), torch.stack(net.drifts)


def cached_eps(sd, cfg, time_of_step, k, full):
    """An eps(net_in, i) callable for tests/ddpm_respace_ref.sample: the network at time_of_step(i) under the schedule, evaluations numbered in
    the order the loop asks for them (predictors and correctors alike).  The CachedNet is the callable's .net."""
    net = CachedNet(sd, cfg, k, full)

    def eps(net_in, i):
        return net(net_in.float(), torch.full((net_in.shape[0],), time_of_step(i), dtype=torch.float32))

    eps.net = net
    return eps
