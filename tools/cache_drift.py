#!/usr/bin/env python3
"""How fast does the cached feature of a checkpoint move?  Runs the Euler sampler with EVERY evaluation full and the drift measurement on
(mi355_feature_cache::drift_out), and prints, per step, the mean and the maximum over the batch of

    ||F_e - F_{e-1}||^2 / ||F_{e-1}||^2,      F = the cached feature of the chosen branch.

Steps where the figure is small are the ones a cache schedule can make shallow; a branch whose figure is large everywhere is cut too deep.
Without --checkpoint the weights are synthetic (seeded): the numbers then only show that the path runs.  Needs an MI355X; there is no
fallback.

    python tools/cache_drift.py --branch 3 [--steps 50] [--batch 64] [--checkpoint PATH] [--precision bf16]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image-inpainting-and-super-resolution-using-diffusion-models-and-conditional-flow-matching_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--branch", type=int, required=True)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--num_channel", type=int, default=128)
    ap.add_argument("--checkpoint", default=None, help="a CIFAR-10 checkpoint of the reference's training script (compute_fid.load_checkpoint)")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("cache_drift needs an MI355X (no fallback)")
    from image_diffusion.unet import param_shapes
    from mi355.synth import synth_state_dict
    from torchcfm_compat import UNetModelWrapper

    dev = torch.device("cuda:0")
    net = UNetModelWrapper(dim=(3, 32, 32), num_res_blocks=2, num_channels=a.num_channel, channel_mult=[1, 2, 2, 2], num_heads=4,
                           num_head_channels=64, attention_resolutions="16", dropout=0.1, precision=a.precision)
    if a.checkpoint:
        from compute_fid import load_checkpoint

        load_checkpoint(net, a.checkpoint)
    else:
        print("no --checkpoint: synthetic weights (the figures show that the path runs, nothing about a trained net)")
        net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
    net.to(dev)
    eng = net.engine(dev)
    branches = eng.cache_branches()
    if not 1 <= a.branch <= len(branches):
        raise SystemExit(f"--branch must be in 1..{len(branches)} for this net")
    b = branches[a.branch - 1]
    print(f"branch {a.branch}: cached feature {b['shape']}, a shallow evaluation keeps {100 * b['retained_flops']:.1f} % of the FLOPs")
    x = torch.randn(a.batch, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(a.seed))
    ts = torch.linspace(0, 1, a.steps + 1).tolist()
    _, _, _, drift = eng.cfm_euler(x, ts, cache_interval=1, cache_branch=a.branch, cache_drift=True)   # every evaluation full: the uncached trajectory
    drift = drift.cpu()
    print(" step      t    mean drift     max drift")
    for e in range(a.steps):
        if float(drift[e, 0]) < 0:
            continue
        print(f"{e:5d} {ts[e]:6.3f}  {float(drift[e].mean()):12.4e}  {float(drift[e].max()):12.4e}")


if __name__ == "__main__":
    main()
