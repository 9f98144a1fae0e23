#!/usr/bin/env python3
"""Times what a learned-variance net costs over a fixed-variance one on the CIFAR configuration: 50-step respaced ancestral sampling at
B = 256, bf16, a 6-output net through mi355_ddpm_lv_sample against a 3-output net through mi355_ddpm_sample_sched.

In ONE process, interleaved round by round.  Each figure is the median of --repeats rounds of a host clock around one synchronised sampler call;
the spread printed beside it is the half range of the 3-output rounds.  The frozen box probe (bench.py's normalisation) runs right behind the
timed rounds.  Then one mi355_unet_profile of an evaluation of each net gives the out conv's device time inside the network and its share of
the evaluation.

    python tools/time_learned_variance.py [--repeats 5] [--out FILE.json]

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
        raise SystemExit("time_learned_variance needs an MI355X (no fallback)")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    B = a.batch
    engs = {}
    for cout in (3, 6):
        net = UNetModel(precision=a.precision, **dict(CIFAR, out_channels=cout))
        net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
        net.to(dev)
        engs[cout] = (net, net.engine(dev))
    r = DDPM(1000).respace(a.steps).with_learned_variance()
    T, ml = r.host_tables(), r.max_log()
    sched = dict(timesteps=r.timesteps, train_steps=r.base_Ns)
    xT = torch.randn(B, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    kw = dict(mode=_lib.DDPM_PRIOR, seed=7, **sched)
    variants = {"fixed_3_outputs": lambda: engs[3][1].ddpm_sample(xT.clone(), T, **kw),
                "learned_6_outputs": lambda: engs[6][1].ddpm_learned(xT.clone(), T, ml, **kw)}
    times = run_rounds(variants, a.repeats)
    box_us = box_probe(L, dev)
    base = times["fixed_3_outputs"]
    doc = {"workload": f"CIFAR net, {a.precision}, B = {B}, {a.steps} respaced ancestral steps of DDPM(1000)", "repeats": a.repeats,
           "box_probe_us": box_us, "box_ref_us": BOX_REF_US, "fixed_half_range_s": (max(base) - min(base)) / 2, "sampler": {}}
    for k, v in times.items():
        med = statistics.median(v)
        doc["sampler"][k] = {"median_s": med, "min_s": min(v), "max_s": max(v), "images_per_s": B / med, "time_vs_fixed": med / statistics.median(base)}
    # the out conv inside the network: per-op device times of one evaluation of each net (the last op is the out conv)
    t = torch.full((B,), 0.5, device=dev)
    doc["out_conv_in_network"] = {}
    for cout, (_, eng) in engs.items():
        eng.profile(xT, t)
        prof = eng.profile(xT, t)
        full_ms = sum(p["ms"] for p in prof)
        last = [p for p in prof if p["kind"] == "conv"][-1]
        doc["out_conv_in_network"][f"128_to_{cout}"] = {"ms": last["ms"], "evaluation_ms": full_ms, "share_of_evaluation": last["ms"] / full_ms,
                                                        "op": {k: last[k] for k in ("kind", "ks", "cin", "cout", "h", "w", "tile")}}
    oc = doc["out_conv_in_network"]
    doc["out_conv_extra_share_of_evaluation"] = (oc["128_to_6"]["ms"] - oc["128_to_3"]["ms"]) / oc["128_to_3"]["evaluation_ms"]
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
