#!/usr/bin/env python3
"""Times feature reuse across sampler steps (DeepCache) on the headline workload: the CIFAR net, bf16, B = 256, 50 Euler steps.

In ONE process, interleaved round by round: engine.cfm_euler without a cache, the cached sampler with every evaluation full, and the cached sampler at
each (interval, branch) asked for.  Each figure is the median of --repeats rounds of a host clock around one synchronised sampler call; the spread
printed beside it is the half range of the uncached rounds of the same run.  The frozen box probe (bench.py's normalisation) runs right behind
the timed rounds.  Then one mi355_unet_profile of a full evaluation gives per-op device times; summed over the plan ops a shallow evaluation
issues they give the predicted time of a cached step, to hold the realised saving against.  With --ddpm the DDPM in-painting workload
(cifar10_inpaint_ddpm50_b512) gets its rows as well.

    python tools/time_feature_cache.py [--repeats 5] [--pairs 2,1 3,3 5,3] [--ddpm] [--out FILE.json]

Needs an MI355X; there is no fallback.  Prints one JSON document (and writes it to --out).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image-inpainting-and-super-resolution-using-diffusion-models-and-conditional-flow-matching_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

BOX_REF_US = 475.0   # bench.py's reference duration of the frozen box probe launch
CIFAR = dict(image_size=32, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(2,),
             channel_mult=(1, 2, 2, 2), num_heads=4, num_head_channels=64)


def box_probe(L, dev):
    import torch

    from mi355 import _lib

    us, mhz, tfl = C.c_float(), C.c_float(), C.c_float()
    pw = torch.empty(int(L.mi355_box_probe_workspace_bytes()), device=dev, dtype=torch.uint8)
    _lib.check(L.mi355_box_probe(20, C.c_void_p(pw.data_ptr()), pw.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(us),
                                 C.byref(mhz), C.byref(tfl)), "mi355_box_probe")
    return float(us.value)


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_rounds(variants, repeats):
    """variants: name -> callable.  One warm-up of each, then `repeats` rounds, every variant once per round in turn.  -> name -> [seconds]."""
    for fn in variants.values():
        timed(fn)
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    return times


def summarise(times, base, B, box_us):
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = (max(times[base]) - min(times[base])) / 2
    rows = {}
    for k, v in times.items():
        rows[k] = {"median_s": med[k], "min_s": min(v), "max_s": max(v), "images_per_s": B / med[k],
                   "images_per_s_box_normalised": B / med[k] * box_us / BOX_REF_US, "time_vs_uncached": med[k] / med[base]}
    return rows, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--pairs", nargs="*", default=["2,1", "3,3", "5,3"], help="interval,branch pairs")
    ap.add_argument("--ddpm", action="store_true", help="also the DDPM in-painting workload (B = 512, 50 steps) at the pairs given by --ddpm-pairs")
    ap.add_argument("--ddpm-pairs", nargs="*", default=["3,3"])
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
        raise SystemExit("time_feature_cache needs an MI355X (no fallback)")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    pairs = [tuple(int(v) for v in p.split(",")) for p in a.pairs]
    doc = {"workload": f"CIFAR net, {a.precision}, B = {a.batch}, {a.steps} Euler steps", "repeats": a.repeats}

    net = UNetModel(precision=a.precision, **CIFAR)
    net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
    net.to(dev)
    eng = net.engine(dev)
    B = a.batch
    x0 = torch.randn(B, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    ts = torch.linspace(0, 1, a.steps + 1).tolist()
    variants = {"uncached": lambda: eng.cfm_euler(x0.clone(), ts, want_u8=True),
                "all_full": lambda: eng.cfm_euler(x0.clone(), ts, want_u8=True, cache_interval=1, cache_branch=1)}
    for n, k in pairs:
        variants[f"interval{n}_branch{k}"] = (lambda n=n, k=k: eng.cfm_euler(x0.clone(), ts, want_u8=True, cache_interval=n, cache_branch=k))
    times = run_rounds(variants, a.repeats)
    box_us = box_probe(L, dev)
    rows, spread = summarise(times, "uncached", B, box_us)
    doc["box_probe_us"] = box_us
    doc["euler"] = rows
    doc["uncached_half_range_s"] = spread
    doc["all_full_within_spread"] = abs(rows["all_full"]["median_s"] - rows["uncached"]["median_s"]) <= max(times["uncached"]) - min(times["uncached"])

    # per-op device times of one full evaluation -> the predicted time of a shallow one
    t = torch.full((B,), 0.5, device=dev)
    eng.profile(x0, t)
    prof = eng.profile(x0, t)
    full_ms = sum(r["ms"] for r in prof)
    branches = {b["branch"]: b for b in eng.cache_branches()}
    pred = {}
    for n, k in pairs:
        lo, hi = branches[k]["skip_ops"]
        shallow_ms = full_ms - sum(r["ms"] for r in prof[1 + lo:1 + hi])
        n_full = sum(1 for e in range(a.steps) if e % n == 0)
        pred_ratio = (n_full * full_ms + (a.steps - n_full) * shallow_ms) / (a.steps * full_ms)
        got_ratio = rows[f"interval{n}_branch{k}"]["time_vs_uncached"]
        pred[f"interval{n}_branch{k}"] = {"full_eval_ms": full_ms, "shallow_eval_ms": shallow_ms, "retained_time_share": shallow_ms / full_ms,
                                          "retained_flop_share": branches[k]["retained_flops"], "predicted_time_vs_uncached": pred_ratio,
                                          "realised_time_vs_uncached": got_ratio,
                                          "realised_over_predicted_saving": (1 - got_ratio) / (1 - pred_ratio) if pred_ratio < 1 else None}
    doc["profile_prediction"] = pred

    if a.ddpm:
        del eng, net
        torch.cuda.empty_cache()
        Bd = 512
        netd = UNetModel(precision=a.precision, **dict(CIFAR, in_channels=6))
        netd.load_state_dict(synth_state_dict(param_shapes(netd), 1234))
        netd.to(dev)
        engd = netd.engine(dev)
        g = torch.Generator(device=dev).manual_seed(0)
        xT = torch.randn(Bd, 3, 32, 32, device=dev, generator=g)
        cond = torch.rand(Bd, 3, 32, 32, device=dev, generator=g) * 2 - 1
        cond[:, :, 8:24, 8:24] = -2.0
        tables = DDPM(50).host_tables()
        kw = dict(mode=_lib.DDPM_AMORTIZED, cond=cond, seed=7)
        vd = {"uncached": lambda: engd.ddpm_sample(xT.clone(), tables, **kw),
              "all_full": lambda: engd.ddpm_sample(xT.clone(), tables, cache_interval=1, cache_branch=1, **kw)}
        for p in a.ddpm_pairs:
            n, k = (int(v) for v in p.split(","))
            vd[f"interval{n}_branch{k}"] = (lambda n=n, k=k: engd.ddpm_sample(xT.clone(), tables, cache_interval=n, cache_branch=k, **kw))
        td = run_rounds(vd, a.repeats)
        box_d = box_probe(L, dev)
        rd, sd_ = summarise(td, "uncached", Bd, box_d)
        doc["ddpm_inpaint_b512"] = {"rows": rd, "uncached_half_range_s": sd_, "box_probe_us": box_d}

    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
