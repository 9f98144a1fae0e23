#!/usr/bin/env python3
"""Cost of per-image x0 shaping (UNetEngine.ddpm_shaped: one statistics launch per predictor step, dynamic thresholding and guidance rescale)
against the PARENT commit's unshaped guided DDIM (UNetEngine.ddpm_sample -> mi355_ddpm_cfg_sample_sched): the CIFAR-10 U-Net (model_channels 128,
6 input channels: state | condition) in bf16 at B = 256, 50 of DDPM(1000)'s steps, guidance scale 4.  Device events around the whole call; within
a process the variants are interleaved round by round.  Every figure is ms per call, except stats_us: the statistics kernel alone, microseconds
per launch over back-to-back launches on the sampler's shapes (eps [512, 3, 32, 32] resident in L2, as behind an evaluation).

The baseline is never the build under test.  The whole measurement is one command, given a checkout of the parent commit with its own
library built (git worktree add ../parent HEAD~1; make -C ../parent/<package>/csrc):

    python tools/time_shaping.py --parent-repo ../parent --out profiles/x0_shaping.json --md profiles/x0_shaping.md

It starts --processes worker processes per side, alternated parent, this, parent, this (the parent's run this file with --repo <parent>
--variants unshaped: its code, its library), pools their rounds and writes the medians, the spreads and the ratios.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

OLD = ("unshaped",)
PKG = "image-inpainting-and-super-resolution-using-diffusion-models-and-conditional-flow-matching_amd"


def merge(this, parent):
    out = {k: this[0][k] for k in ("steps", "rounds", "batch", "config", "shaping")}
    out["processes_per_side"] = {"this": len(this), "parent": len(parent)}
    pool = {k: [t for r in this for t in r["ms_rounds"].get(k, [])] for k in this[0]["ms_rounds"]}
    pool.update({"parent_" + k: [t for r in parent for t in r["ms_rounds"][k]] for k in OLD})
    med = {k: statistics.median(v) for k, v in pool.items()}
    out["ms_median"] = {k: round(v, 3) for k, v in med.items()}
    out["ms_spread"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in pool.items()}
    out["stats_us"] = round(statistics.median([r["stats_us"] for r in this if r.get("stats_us")]), 2)
    out["finite"] = all(r["finite"] for r in this + parent)
    out["ratios"] = {f"{k}_over_parent_unshaped": round(med[k] / med["parent_unshaped"], 4) for k in med if not k.startswith("parent_")}
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


def emit(res, out, md=""):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    if md and "ratios" in res:
        m, sp = res["ms_median"], res["ms_spread"]
        rows = "\n".join(f"| {k} | {m[k]:.3f} | {sp[k][0]:.3f} .. {sp[k][1]:.3f} | {res['ratios'].get(k + '_over_parent_unshaped', 1.0):.4f} |"
                         for k in sorted(m, key=lambda k: (not k.startswith("parent_"), k)))
        with open(md, "w") as f:
            f.write(f"""# Cost of per-image x0 shaping

Measured by `tools/time_shaping.py --parent-repo <parent checkout>` on one MI355X: {res['steps']}-step guided DDIM (guidance scale 4) at
B = {res['batch']} on the CIFAR-10 U-Net ({res['config']}), shaping = {res['shaping']} (quantile, cap, rescale phi).  ms per sampler call, median of
{res['rounds']} rounds x {res['processes_per_side']['this']} processes per side, parent and this build alternated; `parent_unshaped` is the parent
commit's own code and library.

| variant | ms (median) | spread | over parent_unshaped |
|---|---|---|---|
{rows}

The statistics kernel alone (one workgroup per image, B = {res['batch']} images of 3072 elements, guided, operands resident in L2):
{res['stats_us']:.2f} us per launch, back-to-back launches.  Per sampler call that is {res['steps']} launches.

`unshaped` is this build's `ddpm_sample`, `shaped_off` its `ddpm_shaped` with shaping None (both the parent's loop: about 1); `shaped` has both
parts on.  What this says about sample quality: nothing (no trained checkpoint is at hand).
""")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--variants", default="unshaped,shaped_off,shaped")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="", help="with --parent-repo: also write the report as markdown")
    ap.add_argument("--parent-repo", default="", help="a checkout of the parent commit with its library built: run the whole measurement")
    ap.add_argument("--processes", type=int, default=2, help="worker processes per side (with --parent-repo)")
    ap.add_argument("--worker-timeout", type=float, default=240.0)
    a = ap.parse_args()
    if a.parent_repo:
        return emit(drive(a), a.out, a.md)
    sys.path.insert(0, os.path.join(a.repo, PKG))
    import torch

    from image_diffusion.sde_diffusion import DDPM
    from image_diffusion.unet import UNetModel, param_shapes
    from mi355 import _lib
    from mi355.synth import randn, synth_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("time_shaping.py needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")
    kw = dict(image_size=32, in_channels=6, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(2,), channel_mult=(1, 2, 2, 2),
              num_heads=4, num_head_channels=64, precision="bf16")
    net = UNetModel(**kw)
    net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
    eng = net.to(dev).engine(dev)
    r = DDPM(1000).respace(a.steps)
    T = r.host_tables()
    xT = randn(4242, a.batch, 3, 32, 32).to(dev)
    cond = (randn(4243, a.batch, 3, 32, 32) * 0.5).clamp(-1, 1).to(dev)
    shaping = (0.995, None, 0.7)
    call = dict(mode=_lib.DDIM, cond=cond, guidance_scale=4.0, timesteps=r.timesteps, train_steps=r.base_Ns)
    fns = {}
    for v in a.variants.split(","):
        if v == "unshaped":
            fns[v] = lambda x: eng.ddpm_sample(x, T, **call)
        elif v == "shaped_off":
            fns[v] = lambda x: eng.ddpm_shaped(x, T, None, **call)
        else:
            fns[v] = lambda x: eng.ddpm_shaped(x, T, shaping, **call)

    def run(fn):
        x = xT.clone()
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
    res = {"steps": a.steps, "rounds": a.rounds, "batch": a.batch, "config": "cifar_mc128_in6_bf16", "shaping": list(shaping),
           "ms_rounds": {k: [round(t, 3) for t in v] for k, v in ms.items()}, "ms_median": {k: round(statistics.median(v), 3) for k, v in ms.items()},
           "finite": all(bool(torch.isfinite(v).all()) for v in finals.values())}
    if "shaped" in fns:   # the statistics kernel alone, on the sampler's shapes
        from mi355.ops import default_ops as ops

        eps2 = randn(4244, 2 * a.batch, 3, 32, 32).to(dev)
        reps = 50
        for _ in range(5):
            ops.x0_shape_stats(xT, eps2, 1.8, 1.5, shaping, w=4.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.x0_shape_stats(xT, eps2, 1.8, 1.5, shaping, w=4.0)
        e1.record()
        e1.synchronize()
        res["stats_us"] = round(1000.0 * e0.elapsed_time(e1) / reps, 2)
    emit(res, a.out)


if __name__ == "__main__":
    main()
