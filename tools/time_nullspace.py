#!/usr/bin/env python3
"""Cost of the null-space (DDNM) samplers.  Two comparisons, each on one box and in one run:

  loop  50 respaced steps of DDPM(1000) at B = 256 on the CIFAR-10 U-Net (model_channels 128, bf16): NullSpace in the DDIM form (eta 0.85) for the
        mask (kind 0, an 8 x 8 patch unknown) and the block mean (kind 1, factor 4) against the PARENT commit's get_ddim_sample_fn(eta = 0.85) on
        the same chain - the same evaluations, the same draws, one predictor launch per step on either side.  Device events around the whole
        call; within a process the variants are interleaved round by round.  ms per call.
  step  the step launch alone at the loop's n = 256 * 3 * 32 * 32: mi355_nullspace_step of each kind against mi355_pred_step (DDIM(eta)), Philox
        noise on both, `--step-reps` launches between two events; us per launch and achieved bytes per second (x and the output read, x written;
        plus the measurement), next to mi355_box_probe_hbm's copy figure of the same process.

The baseline is never the build under test.  The whole measurement is one command, given a checkout of the parent commit with its own library
built (git worktree add ../parent HEAD~1; make -C ../parent/<package>/csrc):

    python tools/time_nullspace.py --parent-repo ../parent --out profiles/nullspace_timing.json

It starts --processes worker processes per side, alternated parent, this, parent, this (the parent's run this file with --repo <parent> --variants
ddim: its code, its library), pools their rounds and writes the medians, the spreads and the ratios.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

OLD = ("ddim",)


def merge(this, parent):
    out = {k: this[0][k] for k in ("steps", "rounds", "batch", "config")}
    out["processes_per_side"] = {"this": len(this), "parent": len(parent)}
    pool = {k: [t for r in this for t in r["ms_rounds"].get(k, [])] for k in this[0]["ms_rounds"]}
    pool.update({"parent_" + k: [t for r in parent for t in r["ms_rounds"][k]] for k in OLD})
    med = {k: statistics.median(v) for k, v in pool.items()}
    out["ms_median"] = {k: round(v, 3) for k, v in med.items()}
    out["ms_spread"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in pool.items()}
    out["finite"] = all(r["finite"] for r in this + parent)
    out["ratios"] = {f"{k}_over_parent_ddim": round(med[k] / med["parent_ddim"], 4) for k in med if k.startswith("ns_")}
    out["ratios"]["ddim_this_over_parent"] = round(med["ddim"] / med["parent_ddim"], 4) if "ddim" in med else None
    out["step"] = [r["step"] for r in this if r.get("step")]
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
                                "--batch", str(a.batch), "--step-reps", str(a.step_reps), "--out", f], check=True, timeout=a.worker_timeout,
                               stdout=subprocess.DEVNULL)
                files[side].append(json.load(open(f)))
        return merge(files["this"], files["parent"])


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def time_steps(torch, dev, batch, reps):
    """us per launch and achieved GB/s of the step launch alone, and the box's HBM copy figure."""
    from mi355 import _lib
    from mi355.ops import default_ops as ops
    from mi355.synth import randn

    shape = (batch, 3, 32, 32)
    n = batch * 3 * 32 * 32
    x0 = randn(1, *shape).to(dev)
    out = randn(2, *shape).to(dev)
    y_full = (randn(3, *shape) * 0.5).clamp(-1, 1).to(dev)
    y_full[:, :, 12:20, 12:20] = -2.0
    y_low = ops.block_mean(y_full.clip(-1, 1), (8, 8))
    cr, crm1, prev, sigma = 1.9, 1.6, 0.4, 0.3
    launches = {
        "pred_step_ddim_eta": (lambda x, k: ops.pred_step_("ddim_eta", "eps", x, out, cr, crm1, prev, sigma=sigma, philox=(7, 4 * k * n)), 3 * n * 4),
        "nullspace_mask": (lambda x, k: ops.nullspace_step_(ops.nullspace_op(0, pad_value=-2.0), 1, "eps", x, out, y_full, cr, crm1, prev, lam=1.0,
                                                            sigma=sigma, philox=(7, 4 * k * n)), 4 * n * 4),
        "nullspace_block_mean": (lambda x, k: ops.nullspace_step_(ops.nullspace_op(1, y_low.shape), 1, "eps", x, out, y_low, cr, crm1, prev, lam=1.0,
                                                                  sigma=sigma, philox=(7, 4 * k * n)), 3 * n * 4 + n // 16 * 4),
        "nullspace_bilinear": (lambda x, k: ops.nullspace_step_(ops.nullspace_op(2, y_low.shape), 1, "eps", x, out, y_low, cr, crm1, prev, lam=1.0,
                                                                sigma=sigma, philox=(7, 4 * k * n)), 3 * n * 4 + n // 16 * 4),
    }
    res = {"n": n, "reps": reps, "us": {}, "gbytes_per_s": {}, "bytes": {k: b for k, (_, b) in launches.items()}}
    rounds = {k: [] for k in launches}
    for r in range(6):      # the first round warms up
        for name, (fn, _) in launches.items():
            x = x0.clone()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(reps):
                fn(x, k % 8)
            e1.record()
            e1.synchronize()
            if r:
                rounds[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    for name, (_, nbytes) in launches.items():
        us = statistics.median(rounds[name])
        res["us"][name] = round(us, 3)
        res["gbytes_per_s"][name] = round(nbytes / us / 1e3, 1)
    res["us_spread"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in rounds.items()}
    L = _lib.lib()
    wsb = L.mi355_box_probe_hbm_workspace_bytes()
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    us, gb = C.c_float(), C.c_float()
    rc = L.mi355_box_probe_hbm(5, C.c_void_p(ws.data_ptr()), wsb, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(us), C.byref(gb))
    torch.cuda.synchronize()
    if rc == 0 and us.value > 0:
        res["box_probe_hbm"] = {"us_per_launch": round(us.value, 2), "gbytes_moved": round(gb.value, 4),
                                "gbytes_per_s": round(gb.value / (us.value * 1e-6), 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--variants", default="ddim,ns_mask,ns_pool,step")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--step-reps", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-repo", default="", help="a checkout of the parent commit with its library built: run the whole measurement")
    ap.add_argument("--processes", type=int, default=2, help="worker processes per side (with --parent-repo)")
    ap.add_argument("--worker-timeout", type=float, default=240.0)
    a = ap.parse_args()
    if a.parent_repo:
        return emit(drive(a), a.out)
    sys.path.insert(0, os.path.join(a.repo, "image-inpainting-and-super-resolution-using-diffusion-models-and-conditional-flow-matching_amd"))
    import torch

    from image_diffusion import sampling
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM
    from image_diffusion.unet import UNetModel, param_shapes
    from mi355.synth import randn, synth_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("time_nullspace.py needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")
    kw = dict(image_size=32, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(2,), channel_mult=(1, 2, 2, 2),
              num_heads=4, num_head_channels=64, precision="bf16")
    net = UNetModel(**kw)
    net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
    net.to(dev)
    ddpm = DDPM(1000).respace(a.steps)
    eps_model = sampling.make_eps_model(net, ddpm)
    xT = randn(4242, a.batch, 3, 32, 32).to(dev)
    truth = (randn(4243, a.batch, 3, 32, 32) * 0.5).clamp(-1, 1).to(dev)
    variants = a.variants.split(",")
    fns = {}
    if "ddim" in variants:
        ddim = sampling.get_ddim_sample_fn(eps_model, ddpm, eta=0.85)
        fns["ddim"] = lambda: ddim(xT)
    if "ns_mask" in variants or "ns_pool" in variants:
        from image_diffusion.conditioning import NullSpace
        from image_diffusion.likelihoods import AveragePooling

        cnd = NullSpace(0.0, 0.85, 1, 1)
        lik0, lik1 = InPainting(patch_size=8, pad_value=-2), AveragePooling(4)
        y0 = truth.clone()
        y0[:, :, 12:20, 12:20] = -2.0
        y1 = lik1.sample(truth)
        f0 = sampling.get_conditional_sample_fn(eps_model, ddpm, cnd, lik0)
        f1 = sampling.get_conditional_sample_fn(eps_model, ddpm, cnd, lik1)
        if "ns_mask" in variants:
            fns["ns_mask"] = lambda: f0(xT, y0)
        if "ns_pool" in variants:
            fns["ns_pool"] = lambda: f1(xT, y1)

    def run(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        x = fn()
        e1.record()
        e1.synchronize()
        net.engine(dev).check()
        return e0.elapsed_time(e1), x

    for fn in fns.values():   # warm-up: code objects, workspace, every shape of the timed window
        run(fn)
    ms = {k: [] for k in fns}
    finals = {}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            t, finals[k] = run(fn)
            ms[k].append(t)
    step = time_steps(torch, dev, a.batch, a.step_reps) if "step" in variants else None
    emit({"steps": a.steps, "rounds": a.rounds, "batch": a.batch, "config": "cifar_mc128_bf16_ddpm1000_respaced", "step": step,
          "ms_rounds": {k: [round(t, 3) for t in v] for k, v in ms.items()},
          "ms_median": {k: round(statistics.median(v), 3) for k, v in ms.items()},
          "finite": all(bool(torch.isfinite(v).all()) for v in finals.values())}, a.out)


if __name__ == "__main__":
    main()
