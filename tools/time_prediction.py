#!/usr/bin/env python3
"""Times what an x0- or v-prediction chain costs over the eps chain on the CIFAR configuration: 50 respaced ancestral steps and 50 DDIM steps at
B = 256, bf16, the same 3-output net read as each kind (the weights are synthetic: only the arithmetic behind the net differs).

In ONE process, interleaved round by round.  Each figure is the median of --repeats rounds of a host clock around one synchronised sampler call;
the spread printed beside it is the half range of the eps rounds.  The frozen box probe (bench.py's normalisation) runs right behind the timed
rounds.  --eps-only times the eps loops alone through UNetEngine.ddpm_sample: the form that also runs on a tree from before the prediction
kinds, so that such a tree and this one can take turns, a fresh process each.

    python tools/time_prediction.py [--repeats 7] [--eps-only] [--out FILE.json]

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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--eps-only", action="store_true")
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
        raise SystemExit("time_prediction needs an MI355X (no fallback)")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    B = a.batch
    net = UNetModel(precision=a.precision, **CIFAR)
    net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
    net.to(dev)
    eng = net.engine(dev)
    r = DDPM(1000).respace(a.steps)
    T = r.host_tables()
    sched = dict(timesteps=r.timesteps, train_steps=r.base_Ns)
    xT = torch.randn(B, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    modes = {"ancestral": dict(mode=_lib.DDPM_PRIOR, seed=7, **sched), "ddim": dict(mode=_lib.DDIM, **sched)}
    variants = {}
    for loop, kw in modes.items():
        variants[f"{loop}_eps"] = lambda kw=kw: eng.ddpm_sample(xT.clone(), T, **kw)
        if not a.eps_only:
            for kind in ("x0", "v"):
                variants[f"{loop}_{kind}"] = lambda kw=kw, kind=kind: eng.ddpm_sample(xT.clone(), T, prediction=kind, **kw)
    times = run_rounds(variants, a.repeats)
    box_us = box_probe(L, dev)
    doc = {"workload": f"CIFAR net, {a.precision}, B = {B}, {a.steps} respaced steps of DDPM(1000)", "repeats": a.repeats, "box_probe_us": box_us,
           "box_ref_us": BOX_REF_US, "launches_last_evaluation_and_step": {}, "sampler": {}}
    for loop in modes:
        base = times[f"{loop}_eps"]
        doc[f"{loop}_eps_half_range_s"] = (max(base) - min(base)) / 2
        for k, v in times.items():
            if k.startswith(loop + "_"):
                med = statistics.median(v)
                doc["sampler"][k] = {"median_s": med, "min_s": min(v), "max_s": max(v), "images_per_s": B / med,
                                     "time_vs_eps": med / statistics.median(base)}
    for k, fn in variants.items():      # what mi355_unet_get_stats reports after a call: the last evaluation (+ its step, where the entry point counts it)
        fn()
        doc["launches_last_evaluation_and_step"][k] = eng.stats(B)["launches"]
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
