#!/usr/bin/env python3
"""Generate tests/golden/unet_*_classcond.npz: class-conditional reference U-Nets (UNetModel(num_classes=K), build container only).

Reuses the helpers of tools/make_goldens.py (the reference's own modules, synthesised weights).  Each fixture holds the reference's
state_dict key list (label_emb.weight [K, 4*model_channels] right after time_embed.2.bias), the inputs x, t and the reference output.
The reference's forward(x, timesteps) never reads label_emb (AD/image_diffusion/unet.py:708-728), so the output is the y=None behaviour;
the label term itself has no reference fixture (tests/test_gpu_classcond.py restates it).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402

CASES = {
    # name: (base case of make_goldens.UNET_CASES, num_classes, batch, seed)
    "tiny": ("tiny_in3", 5, 3, 3001),
    "tiny_film_updown_neworder": ("tiny_film_updown_neworder", 5, 3, 3005),
    "mnist": ("mnist", 10, 3, 3010),
}


def main():
    for name, (base, K, B, seed) in CASES.items():
        kw = dict(mg.UNET_CASES[base][0], num_classes=K)
        net = mg.load_synth(mg.make_unet(**kw), seed)
        keys = [[k, list(v.shape)] for k, v in net.state_dict().items()]
        x = mg.randn(seed + 50000, B, kw["in_channels"], kw["image_size"], kw["image_size"])
        t = torch.tensor([0.37, 0.91, 0.0, 1.0][:B])
        y = net(x, t)
        cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
        mg.save(f"unet_{name}_classcond", x=x, t=t, y=y, keys=keys, config=cfg, seed=np.int64(seed), num_classes=np.int64(K),
                n_params=np.int64(sum(p.numel() for p in net.parameters())))


if __name__ == "__main__":
    main()
