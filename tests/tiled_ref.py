"""Restatement of tiled sampling (MultiDiffusion: Bar-Tal et al., ICML 2023) on the oracle U-Net (TEST ORACLE; no reference counterpart).  Built
from oracle.unet_ref's build_plan, _run_layers, timestep_embedding and group_norm32 (the embedding taken the way tests/feature_cache_ref.py::_emb
takes it, so class labels fit in), independently of csrc / mi355.

A canvas [B, C, Hc, Wc] with Hc, Wc >= S = cfg.image_size is cut into overlapping S x S windows.  Along an axis of length L with stride s there
are n = ceil((L - S) / s) + 1 windows at o_i = min(i * s, L - S).  Windows are ordered row-major over (iy, ix); window w of canvas b is batch row
b * nW + w.  The net's predictions are fused per pixel by the weighted average sum_w weight_w v_w / sum_w weight_w with separable weights
p(dy) p(dx): "uniform" p = 1, "tent" p(i) = min(i + 1, S - i).  The network runs in fp32 (as the oracle does); the blend of tiled_eval and the
sampler loops around it run in fp64.  blend_fp32 is the same average as the eager fp32 expression in the order the kernel is held to.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import unet_ref
from tests import ddpm_respace_ref as DR
from tests.feature_cache_ref import _emb


def axis_origins(L: int, S: int, s: int):
    assert L >= S and 1 <= s <= S, (L, S, s)
    n = math.ceil((L - S) / s) + 1
    return [min(i * s, L - S) for i in range(n)]


def origins(canvas_hw, S: int, stride):
    """-> (oy, ox): the window origins along each axis.  stride: an int or (sy, sx)."""
    sy, sx = (stride, stride) if isinstance(stride, int) else stride
    return axis_origins(canvas_hw[0], S, sy), axis_origins(canvas_hw[1], S, sx)


def window_list(canvas_hw, S: int, stride):
    """The (oy, ox) of every window in batch order."""
    oy, ox = origins(canvas_hw, S, stride)
    return [(a, b) for a in oy for b in ox]


def taper(S: int, weight: str, dtype=torch.float64):
    if weight == "uniform":
        return torch.ones(S, dtype=dtype)
    assert weight == "tent", weight
    return torch.tensor([min(i + 1, S - i) for i in range(S)], dtype=dtype)


def weight_map(S: int, weight: str, dtype=torch.float64):
    p = taper(S, weight, dtype)
    return p[:, None] * p[None, :]


def cut(x, S: int, stride):
    """canvas [B, C, Hc, Wc] -> windows [B * nW, C, S, S] by slicing."""
    wl = window_list(x.shape[-2:], S, stride)
    return torch.stack([x[:, :, a:a + S, b:b + S] for a, b in wl], dim=1).reshape(x.shape[0] * len(wl), x.shape[1], S, S)


def blend(v_windows, canvas_hw, stride, weight, *, last_wins=False):
    """windows [B * nW, C, S, S] -> the weighted average on the canvas, in the windows' dtype (fp64 in the loops).  last_wins: the
    discrimination alternative in which a later window overwrites the earlier ones."""
    S = v_windows.shape[-1]
    wl = window_list(canvas_hw, S, stride)
    B = v_windows.shape[0] // len(wl)
    v = v_windows.reshape(B, len(wl), v_windows.shape[1], S, S)
    num = torch.zeros(B, v.shape[2], *canvas_hw, dtype=v.dtype)
    den = torch.zeros(canvas_hw, dtype=v.dtype)
    w = weight_map(S, weight, v.dtype)
    for k, (a, b) in enumerate(wl):
        if last_wins:
            num[:, :, a:a + S, b:b + S] = v[:, k]
            den[a:a + S, b:b + S] = 1
        else:
            num[:, :, a:a + S, b:b + S] += w * v[:, k]
            den[a:a + S, b:b + S] += w
    return num / den


def blend_fp32(v_windows, plan, x=None, dt=None):
    """The eager fp32 expression in the contract's order: windows ascending, num[sl] += w * v, den[sl] += w; then num / den; then x + dt * vbar.
    plan: dict(canvas_hw, stride, weight).  -> vbar, or (vbar, x + dt * vbar).  Runs on v_windows' device."""
    canvas_hw, stride, weight = plan["canvas_hw"], plan["stride"], plan["weight"]
    S = v_windows.shape[-1]
    wl = window_list(canvas_hw, S, stride)
    B = v_windows.shape[0] // len(wl)
    v = v_windows.float().reshape(B, len(wl), v_windows.shape[1], S, S)
    num = torch.zeros(B, v.shape[2], *canvas_hw, dtype=torch.float32, device=v.device)
    den = torch.zeros(canvas_hw, dtype=torch.float32, device=v.device)
    w = weight_map(S, weight, torch.float32).to(v.device)
    for k, (a, b) in enumerate(wl):
        num[:, :, a:a + S, b:b + S] += w * v[:, k]
        den[a:a + S, b:b + S] += w
    vbar = num / den
    if x is None:
        return vbar
    return vbar, x + torch.tensor(dt, dtype=torch.float32, device=v.device) * vbar


@torch.no_grad()
def net_forward(sd, cfg, x, t, y=None):
    """UNetModel.forward(x, t[, y]) in fp32 on the oracle's layers."""
    input_blocks, middle, output_blocks, _ = unet_ref.build_plan(cfg)
    emb = _emb(sd, cfg, t, y)
    hs, h = [], x.float()
    for i, layers in enumerate(input_blocks):
        h = unet_ref._run_layers(sd, cfg, f"input_blocks.{i}", layers, h, emb)
        hs.append(h)
    h = unet_ref._run_layers(sd, cfg, "middle_block", middle, h, emb)
    for i, layers in enumerate(output_blocks):
        h = unet_ref._run_layers(sd, cfg, f"output_blocks.{i}", layers, torch.cat([h, hs.pop()], dim=1), emb)
    return unet_ref._conv(sd, "out.2", F.silu(unet_ref.group_norm32(h, sd["out.0.weight"], sd["out.0.bias"])))


def tiled_eval(sd, cfg, x, t, stride, weight, cond=None, y=None, *, last_wins=False):
    """One tiled evaluation at the time t (a float): fp32 net on the windows of x (| cond), fp64 blend -> [B, out_channels, Hc, Wc] fp64.
    y: one label per canvas."""
    S = cfg.image_size
    xin = x.float() if cond is None else torch.cat((x.float(), cond.float()), dim=1)
    win = cut(xin, S, stride)
    nW = win.shape[0] // x.shape[0]
    yw = None if y is None else y.repeat_interleave(nW)
    v = net_forward(sd, cfg, win, torch.full((win.shape[0],), float(t), dtype=torch.float32), yw)
    return blend(v.double(), tuple(x.shape[-2:]), stride, weight, last_wins=last_wins)


def tiled_euler(sd, cfg, x0, t_span, stride, weight, cond=None, y=None, *, last_wins=False, dtype=torch.float64):
    """oracle.cfm_ref.euler_trajectory around the tiled evaluation, the state and the step in `dtype`: fp64 (the reference the GPU loops are held
    to), or fp32 (the oracle's own arithmetic: with one window it IS oracle.cfm_ref.euler_trajectory, bit for bit).  t_span: fp32 values (the
    differences are taken in fp32, as the sampler takes them).  -> all len(t_span) states [n_t, B, C, Hc, Wc] in dtype."""
    ts = torch.as_tensor(t_span, dtype=torch.float32)
    x = x0.to(dtype)
    xs = [x]
    for j in range(len(ts) - 1):
        v = tiled_eval(sd, cfg, x, float(ts[j]), stride, weight, cond, y, last_wins=last_wins)
        x = x + (ts[j + 1] - ts[j]).to(dtype) * v.to(dtype)
        xs.append(x)
    return torch.stack(xs)


def tiled_eps(sd, cfg, time_of_step, stride, weight):
    """An eps(net_in, i) callable for tests/ddpm_respace_ref.sample: the tiled evaluation at time_of_step(i).  net_in is the canvas state, or
    state | condition for an amortized net (the loop concatenates them), so the loops of that file run tiled with the evaluation swapped."""
    def eps(net_in, i):
        return tiled_eval(sd, cfg, net_in, time_of_step(i), stride, weight)

    return eps


def tiled_ddpm(sd, cfg, time_of_step, T, xT, noise, stride, weight, **kw):
    """tests/ddpm_respace_ref.sample (prior, amortized, replacement, ddim; correctors and walks) on canvases.  -> (x0, draws used, evaluations)."""
    return DR.sample(tiled_eps(sd, cfg, time_of_step, stride, weight), T, xT, noise, **kw)
