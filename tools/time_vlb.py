#!/usr/bin/env python3
"""Times the variational-bound evaluation against ancestral sampling of the same chain on the CIFAR configuration: 50 respaced steps of
DDPM(1000) at B = 256, bf16, a 6-output net (learned variance) and a 3-output net (fixed variance).  A bound step is one evaluation plus two
streaming launches (the noising and the terms kernel), which is what an ancestral step costs (one evaluation plus the step kernel), so the
ratio is expected near 1; the ancestral loops are the yardstick.

In ONE process, interleaved round by round.  Each figure is the median of --repeats rounds of a host clock around one synchronised call; the
spread printed beside it is the half range of the 3-output ancestral rounds.  The frozen box probe (bench.py's normalisation) runs right behind
the timed rounds.  The launch counts are what mi355_unet_get_stats reports after each call (the last evaluation with its step's launches).

    python tools/time_vlb.py [--repeats 5] [--out FILE.json]

Needs an MI355X; there is no fallback.  Prints one JSON document (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from time_feature_cache import BOX_REF_US, CIFAR, box_probe, run_rounds  # noqa: E402  (also puts the package on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians)")

    import torch

    from image_diffusion.sde_diffusion import DDPM
    from image_diffusion.unet import UNetModel, param_shapes
    from mi355 import _lib
    from mi355.synth import synth_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("time_vlb needs an MI355X (no fallback)")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    B = a.batch
    engs = {}
    for cout in (3, 6):
        net = UNetModel(precision=a.precision, **dict(CIFAR, out_channels=cout))
        net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
        net.to(dev)
        engs[cout] = net.engine(dev)
    r = DDPM(1000).respace(a.steps).with_learned_variance()
    T, ml = r.host_tables(), r.max_log()
    learned, fixed = r.vlb_log_variances("learned"), r.vlb_log_variances("fixed_small")
    times_k = torch.tensor([r.time(k) for k in range(r.Ns)], dtype=torch.float32)
    sched = dict(timesteps=r.timesteps, train_steps=r.base_Ns)
    g = torch.Generator(device=dev).manual_seed(0)
    xT = torch.randn(B, 3, 32, 32, device=dev, generator=g)
    x0 = (torch.randint(0, 256, (B, 3, 32, 32), device=dev, generator=g).float() / 127.5 - 1.0).contiguous()
    kw = dict(mode=_lib.DDPM_PRIOR, seed=7, **sched)
    variants = {"ancestral_3_outputs": lambda: engs[3].ddpm_sample(xT.clone(), T, **kw),
                "vlb_fixed_3_outputs": lambda: engs[3].ddpm_vlb(x0, T, fixed, learned=False, times=times_k, seed=7),
                "ancestral_6_outputs": lambda: engs[6].ddpm_learned(xT.clone(), T, ml, **kw),
                "vlb_learned_6_outputs": lambda: engs[6].ddpm_vlb(x0, T, learned, learned=True, times=times_k, seed=7)}
    times = run_rounds(variants, a.repeats)
    box_us = box_probe(L, dev)
    base = times["ancestral_3_outputs"]
    doc = {"workload": f"CIFAR net, {a.precision}, B = {B}, {a.steps} respaced steps of DDPM(1000)", "repeats": a.repeats,
           "box_probe_us": box_us, "box_ref_us": BOX_REF_US, "ancestral_3_half_range_s": (max(base) - min(base)) / 2, "calls": {}}
    for k, v in times.items():
        med = statistics.median(v)
        doc["calls"][k] = {"median_s": med, "min_s": min(v), "max_s": max(v), "images_per_s": B / med}
    for cout, kind in ((3, "fixed"), (6, "learned")):
        doc[f"vlb_over_ancestral_{cout}_outputs"] = doc["calls"][f"vlb_{kind}_{cout}_outputs"]["median_s"] / doc["calls"][f"ancestral_{cout}_outputs"]["median_s"]
    # launches of the last evaluation with its step: sched / lv sampling counts what its entry point counts, the bound its two extra launches
    doc["launches_last_step"] = {}
    for name, fn in variants.items():
        fn()
        torch.cuda.synchronize()
        doc["launches_last_step"][name] = int(engs[3 if "_3_" in name else 6].stats(B)["launches"])
    terms, summary = variants["vlb_learned_6_outputs"]()
    doc["untrained_net_total_bpd_mean"] = float(summary[:, 1].mean())   # a synthetic net: the number says nothing about a model
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
