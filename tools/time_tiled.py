#!/usr/bin/env python3
"""Times tiled sampling (MultiDiffusion) against the untiled sampler at the same network batch: the CIFAR net, bf16, 50 Euler steps.

    tiled    engine.cfm_euler(tiling=) on 28 canvases of 64 x 64 at stride 16: 9 windows per canvas, 252 windows per evaluation
    untiled  engine.cfm_euler on B = 252 images of 32 x 32 (the same 252 forwards' worth of network per step)

In ONE process, the two alternating round by round, each call between two device events on the current stream; one warm-up of each first.  Each
figure is the median of --repeats rounds; the spread printed beside it is the half range of the untiled rounds.  The tiled loop adds two HBM-bound
launches per step (gather, blend) and takes the Euler update out of the last conv's epilogue; the bytes those two launches move are computed
from the shapes.  With --profile, one mi355_unet_profile of a forward at the window batch itemises where an evaluation's time goes.

    python tools/time_tiled.py [--repeats 7] [--canvases 28] [--canvas 64] [--stride 16] [--steps 50] [--profile] [--out FILE.json]

Needs an MI355X; there is no fallback.  Prints one JSON document (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image-inpainting-and-super-resolution-using-diffusion-models-and-conditional-flow-matching_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

CIFAR = dict(image_size=32, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(2,),
             channel_mult=(1, 2, 2, 2), num_heads=4, num_head_channels=64)


def timed_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--canvases", type=int, default=28)
    ap.add_argument("--canvas", type=int, default=64)
    ap.add_argument("--stride", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--weight", default="uniform")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5 (medians)")

    import torch

    from image_diffusion.unet import UNetModel, param_shapes
    from mi355.synth import synth_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("time_tiled needs an MI355X (no fallback)")
    dev = torch.device("cuda:0")
    net = UNetModel(precision=a.precision, **CIFAR)
    net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
    net.to(dev)
    eng = net.engine(dev)
    S, Hc = CIFAR["image_size"], a.canvas
    tp = eng.tile_plan((Hc, Hc), a.stride, a.weight)
    nW = tp["n_windows"]
    rows = a.canvases * nW
    g = torch.Generator(device=dev).manual_seed(0)
    canvas = torch.randn(a.canvases, 3, Hc, Hc, device=dev, generator=g)
    images = torch.randn(rows, 3, S, S, device=dev, generator=g)
    ts = torch.linspace(0, 1, a.steps + 1).tolist()
    tiling = dict(stride=a.stride, weight=a.weight)
    variants = {"untiled": lambda: eng.cfm_euler(images.clone(), ts, want_u8=True),
                "tiled": lambda: eng.cfm_euler(canvas.clone(), ts, want_u8=True, tiling=tiling)}
    for fn in variants.values():
        timed_ms(fn)
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, fn in variants.items():
            times[k].append(timed_ms(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    win_bytes = rows * 3 * S * S * 4
    can_bytes = a.canvases * 3 * Hc * Hc * 4
    doc = {"workload": f"CIFAR net, {a.precision}, {a.steps} Euler steps; tiled: {a.canvases} canvases of {Hc} x {Hc} at stride {a.stride} "
                       f"({nW} windows each, {rows} per evaluation, weight {a.weight}); untiled: B = {rows}",
           "repeats": a.repeats,
           "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
           "untiled_half_range_ms": (max(times["untiled"]) - min(times["untiled"])) / 2,
           "tiled_over_untiled": med["tiled"] / med["untiled"],
           "extra_ms_per_step": (med["tiled"] - med["untiled"]) / a.steps,
           "bytes_per_evaluation_from_shapes": {"gather_read_canvas": can_bytes, "gather_write_windows": win_bytes,
                                                "blend_read_windows": win_bytes, "blend_write_vbar": can_bytes,
                                                "blend_read_write_x": 2 * can_bytes}}
    if a.profile:
        t = torch.full((rows,), 0.5, device=dev)
        eng.profile(images, t)
        prof = eng.profile(images, t)
        by_kind = {}
        for r in prof:
            by_kind[r["kind"]] = by_kind.get(r["kind"], 0.0) + r["ms"]
        doc["forward_profile_ms_at_window_batch"] = {"total": sum(r["ms"] for r in prof), "by_kind": by_kind,
                                                     "last_conv": next((r["ms"] for r in reversed(prof) if r["kind"] == "conv"), None)}
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
