#!/usr/bin/env python3
"""Cost of the Adams-Bashforth CFM samplers (UNetEngine.cfm_ab: one evaluation per step after the start steps) against the PARENT commit's
cfm_euler (n evaluations) and cfm_rk("midpoint") (2n evaluations) over the same n steps: the CIFAR-10 U-Net (model_channels 128) in bf16 at
B = 256, n = 50 steps of linspace(0, 1, n + 1).  Device events around the whole call; within a process the variants are interleaved round by
round.  Every figure is ms per call.

The baseline is never the build under test.  The whole measurement is one command, given a checkout of the parent commit with its own
library built (git worktree add ../parent HEAD~1; make -C ../parent/<package>/csrc):

    python tools/time_multistep.py --parent-repo ../parent --out profiles/multistep_timing.json

It starts --processes worker processes per side, alternated parent, this, parent, this (the parent's run this file with --repo <parent>
--variants euler,midpoint: its code, its library), pools their rounds and writes the medians, the spreads and the ratios of each AB sampler
to the parent's Euler and midpoint calls, and of this build's Euler and midpoint to the parent's (no existing path changed: about 1).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

OLD = ("euler", "midpoint")


def merge(this, parent):
    out = {k: this[0][k] for k in ("steps", "rounds", "batch", "config")}
    out["processes_per_side"] = {"this": len(this), "parent": len(parent)}
    pool = {k: [t for r in this for t in r["ms_rounds"].get(k, [])] for k in this[0]["ms_rounds"]}
    pool.update({"parent_" + k: [t for r in parent for t in r["ms_rounds"][k]] for k in OLD})
    med = {k: statistics.median(v) for k, v in pool.items()}
    out["ms_median"] = {k: round(v, 3) for k, v in med.items()}
    out["ms_spread"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in pool.items()}
    out["finite"] = all(r["finite"] for r in this + parent)
    out["ratios"] = {f"{k}_over_parent_{o}": round(med[k] / med["parent_" + o], 4) for k in med if k.startswith("ab") for o in OLD}
    out["ratios"].update({f"{o}_this_over_parent": round(med[o] / med["parent_" + o], 4) for o in OLD if o in med})
    return out


def drive(a):
    """Alternate worker processes of the parent checkout and of this one (this process never opens the device); stop at the first failure."""
    here = os.path.abspath(__file__)
    files = {"parent": [], "this": []}
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(a.processes):
            for side, repo, variants in (("parent", os.path.abspath(a.parent_repo), ",".join(OLD)), ("this", a.repo, a.variants)):
                f = os.path.join(tmp, f"{side}{i}.json")
                subprocess.run([sys.executable, here, "--repo", repo, "--variants", variants, "--steps", str(a.steps), "--rounds", str(a.rounds),
                                "--batch", str(a.batch), "--out", f], check=True, timeout=a.worker_timeout, stdout=subprocess.DEVNULL)
                files[side].append(json.load(open(f)))
        return merge(files["this"], files["parent"])


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--variants", default="euler,midpoint,ab2,ab3,ab4")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-repo", default="", help="a checkout of the parent commit with its library built: run the whole measurement")
    ap.add_argument("--processes", type=int, default=2, help="worker processes per side (with --parent-repo)")
    ap.add_argument("--worker-timeout", type=float, default=240.0)
    a = ap.parse_args()
    if a.parent_repo:
        return emit(drive(a), a.out)
    sys.path.insert(0, os.path.join(a.repo, "image-inpainting-and-super-resolution-using-diffusion-models-and-conditional-flow-matching_amd"))
    import torch

    from image_diffusion.unet import UNetModel, param_shapes
    from mi355.synth import randn, synth_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("time_multistep.py needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")
    kw = dict(image_size=32, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(2,), channel_mult=(1, 2, 2, 2),
              num_heads=4, num_head_channels=64, precision="bf16")
    net = UNetModel(**kw)
    net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
    eng = net.to(dev).engine(dev)
    ts = torch.linspace(0, 1, a.steps + 1).tolist()
    x0 = randn(4242, a.batch, 3, 32, 32).to(dev)
    fns = {}
    for v in a.variants.split(","):
        if v == "euler":
            fns[v] = lambda x: eng.cfm_euler(x, ts)
        elif v == "midpoint":
            fns[v] = lambda x: eng.cfm_rk(x, ts, "midpoint")
        else:
            fns[v] = lambda x, v=v: eng.cfm_ab(x, ts, v)

    def run(fn):
        x = x0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(x)
        e1.record()
        e1.synchronize()
        eng.check()
        return e0.elapsed_time(e1), x

    for fn in fns.values():   # warm-up: code objects, workspace, every shape of the timed window
        run(fn)
    ms = {k: [] for k in fns}
    finals = {}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            t, finals[k] = run(fn)
            ms[k].append(t)
    emit({"steps": a.steps, "rounds": a.rounds, "batch": a.batch, "config": "cifar_mc128_bf16", "ms_rounds": {k: [round(t, 3) for t in v] for k, v in ms.items()},
          "ms_median": {k: round(statistics.median(v), 3) for k, v in ms.items()},
          "finite": all(bool(torch.isfinite(v).all()) for v in finals.values())}, a.out)


if __name__ == "__main__":
    main()
