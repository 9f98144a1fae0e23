#!/usr/bin/env python3
"""Cost of class-conditional sampling: the CIFAR-10 U-Net (model_channels 128, BASELINE cfg 2 geometry) with num_classes = 10 in bf16 at
B = 256, Euler steps through UNetEngine.cfm_euler, timed with device events in one process, the variants interleaved round by round:

  uncond   cfm_euler(x, t_span)         - the unconditional loop (label_emb unread, the precomputed time-embedding table)
  table    cfm_euler(x, t_span, y=y)    - 50 steps x 10 classes <= 1024 rows: the (step, class) table, one row gather per step
  fallback cfm_euler(x, t_span, y=y)    - 103 steps x 10 classes > 1024 rows: each step computes its rows (label_emb_linear over B rows)

`table` is compared with `uncond` over 50 steps, `fallback` with `uncond` over 103 steps; every figure is per network evaluation.
Prints one JSON line; --out also writes it to a file.
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

from image_diffusion.unet import UNetModel, param_shapes  # noqa: E402
from mi355.synth import randn, synth_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_classcond.py needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")
    K = 10
    net = UNetModel(image_size=32, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(2,),
                    channel_mult=(1, 2, 2, 2), num_heads=4, num_head_channels=64, num_classes=K, precision=a.precision)
    net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
    net.to(dev)
    eng = net.engine(dev)
    B = a.batch
    x0 = randn(4242, B, 3, 32, 32).to(dev)
    y = (torch.arange(B) % K).to(dev)
    spans = {50: torch.linspace(0, 1, 51).tolist(), 103: torch.linspace(0, 1, 104).tolist()}
    variants = {"uncond50": (50, None), "table50": (50, y), "uncond103": (103, None), "fallback103": (103, y)}

    def run(name):
        n, lab = variants[name]
        x = x0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.cfm_euler(x, spans[n], y=lab)
        e1.record()
        e1.synchronize()
        eng.check()
        return e0.elapsed_time(e1) / n, eng.stats(B)["launches"], x

    for name in variants:   # warm-up: code objects, workspace, every shape of the timed window
        run(name)
    ms = {k: [] for k in variants}
    launches = {}
    finals = {}
    for _ in range(a.rounds):
        for name in variants:
            t, nl, x = run(name)
            ms[name].append(t)
            launches[name] = nl
            finals[name] = x
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {
        "config": "cifar mc128 B=%d %s K=%d" % (B, a.precision, K),
        "ms_per_eval_median": {k: round(v, 4) for k, v in med.items()},
        "ms_per_eval_spread": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "table_over_uncond_pct": round(100.0 * (med["table50"] / med["uncond50"] - 1.0), 2),
        "fallback_over_uncond_us": round(1000.0 * (med["fallback103"] - med["uncond103"]), 1),
        "launches_per_step_last": launches,
        "labels_change_output": bool((finals["table50"] - finals["uncond50"]).abs().max().item() > 1e-3),
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
