"""Drop-in for the sampler half of the reference's `cifar10/compute_fid.py` on the MI355X backend.

`make_gen_1_img` builds the `gen_1_img(unused_latent) -> uint8 [B,3,32,32]` closure that cleanfid's
`fid.compute_fid(gen=...)` calls (cifar10/compute_fid.py:73-88), with the same flag names
(`integration_steps`, `integration_method`, `batch_size_fid`, `num_channel`).  With world_size > 1 every rank
samples its shard and the shards are collected with ONE RCCL all-gather (mi355.dist).  cleanfid itself
(Inception weights + CIFAR statistics, both downloaded) is not available offline; `main()` reports that.
"""
import argparse
import os

import torch

from mi355 import dist as mdist
from torchcfm_compat import ClassCondUNetModelWrapper, UNetModelWrapper


def build_model(num_channel=128, device="cuda:0", precision=None, num_classes=None):
    """cifar10/compute_fid.py:39-48.  num_classes: the class-conditional form of the same net (for --guidance_scale)."""
    kw = dict(dim=(3, 32, 32), num_res_blocks=2, num_channels=num_channel, channel_mult=[1, 2, 2, 2], num_heads=4, num_head_channels=64,
              attention_resolutions="16", dropout=0.1, precision=precision)
    if num_classes:
        return ClassCondUNetModelWrapper(class_cond=True, num_classes=int(num_classes), **kw).to(device)
    return UNetModelWrapper(**kw).to(device)


def load_checkpoint(net, path):
    """cifar10/compute_fid.py:52-65: take ["ema_model"], strip a 7-char "module." prefix on mismatch."""
    checkpoint = torch.load(path, map_location="cpu", weights_only=True)
    state_dict = checkpoint["ema_model"]
    try:
        net.load_state_dict(state_dict)
    except RuntimeError:
        net.load_state_dict({k[7:]: v for k, v in state_dict.items()})
    net.eval()
    return net


def draw_x0_shard(batch, seed, call_idx, device, shape=(3, 32, 32)):
    """This rank's slice of the batch's initial noise.  Every rank draws the SAME [batch, *shape] tensor from a generator seeded
    with seed + call_idx and keeps rows shard_range(batch), so an N-rank run integrates exactly the x0 of the 1-rank run
    (the reference's single `torch.randn(batch_size_fid, 3, 32, 32)`, cifar10/compute_fid.py:75, re-sharded)."""
    lo, hi = mdist.shard_range(batch)
    g = torch.Generator(device=device)
    g.manual_seed(int(seed) + int(call_idx))
    return torch.randn(batch, *shape, device=device, generator=g)[lo:hi].contiguous()


def make_gen_1_img(new_net, batch_size_fid=1024, integration_steps=100, integration_method="euler", device="cuda:0", tol=1e-5, seed=0,
                   guidance_scale=None, null_label=None, cache_interval=None, cache_branch=None):
    """cache_interval / cache_branch (None: every step evaluates the whole net): feature reuse across the Euler steps (DeepCache; one full
    evaluation in cache_interval, the cache_branch outermost block pairs recomputed at every step: UNetEngine.cfm_euler); Euler only, unguided.
    guidance_scale (None: unguided, the reference's call): classifier-free guidance on a class-conditional net; each image's label is drawn
    uniformly from the classes other than null_label (default: the last class) by the batch's seeded generator.
    integration_method: "euler", "dopri5", a fixed-step Runge-Kutta name ("midpoint", "heun2", "rk4", "rk4_38": mi355.ode.TABLEAUS) or an
    Adams-Bashforth name ("ab2", "ab3", "ab4": mi355.ode.AB_SOLVERS).
    The fixed-step methods integrate over linspace(0, 1, integration_steps + 1) like the Euler branch - a build-defined reading: the
    reference forwards any name but "euler" to odeint with the two-point grid linspace(0, 1, 2), which for a fixed-grid method is ONE
    step over [0, 1]."""
    from mi355.ode import AB_SOLVERS as ab, RK_SOLVERS as rk

    if integration_method not in ("euler", "dopri5") + rk + ab:
        raise NotImplementedError(f"--integration_method must be euler, dopri5 or one of {rk + ab}")
    cache = {}
    if cache_interval is not None or cache_branch is not None:
        if integration_method != "euler":
            raise NotImplementedError("--cache_interval / --cache_branch are built for --integration_method euler only")
        cache = dict(cache_interval=1 if cache_interval is None else int(cache_interval), cache_branch=cache_branch)
    device = torch.device(device)
    calls = [0]
    guide = {}
    if guidance_scale is not None:
        K = getattr(new_net, "num_classes", None)
        if not K:
            raise ValueError("--guidance_scale needs a class-conditional model (num_classes)")
        nl = K - 1 if null_label is None else int(null_label)
        if not 0 <= nl < K:
            raise ValueError(f"--null_label must be a class index in [0, {K})")
        guide = dict(guidance_scale=float(guidance_scale), null_label=nl)

    def draw_labels(B, call_idx):
        lo, hi = mdist.shard_range(B)
        g = torch.Generator(device="cpu")
        g.manual_seed(int(seed) + int(call_idx) + (1 << 20))
        y = torch.randint(0, new_net.num_classes - 1, (B,), generator=g)
        return (y + (y >= guide["null_label"]).long())[lo:hi].to(device)

    def gen_1_img(unused_latent):
        with torch.no_grad():
            B = int(batch_size_fid)
            x = draw_x0_shard(B, seed, calls[0], device)
            kw = dict(guide, y=draw_labels(B, calls[0])) if guide else {}
            calls[0] += 1
            if integration_method == "euler":
                t_span = torch.linspace(0, 1, integration_steps + 1).tolist()
                _, _, img = new_net.engine(device).cfm_euler(x, t_span, want_u8=True, **kw, **cache)  # (traj*127.5+128).clip(0,255).to(uint8)
            elif integration_method in rk:
                t_span = torch.linspace(0, 1, integration_steps + 1).tolist()
                _, _, img = new_net.engine(device).cfm_rk(x, t_span, integration_method, want_u8=True, **kw)
            elif integration_method in ab:   # Adams-Bashforth on the same grid: one evaluation per step after the start steps
                t_span = torch.linspace(0, 1, integration_steps + 1).tolist()
                _, _, img = new_net.engine(device).cfm_ab(x, t_span, integration_method, want_u8=True, **kw)
            else:  # odeint(new_net, x, linspace(0,1,2), rtol=tol, atol=tol, method="dopri5")  (cifar10/compute_fid.py:80-85)
                from mi355.ode import odeint_dopri5
                from mi355.ops import default_ops

                # guided: model(t, x, y, guidance_scale=, null_label=), the 2B forward plus cfg_stage per evaluation
                traj, _ = odeint_dopri5(lambda t, xt: new_net(torch.tensor(float(t), device=device), xt, **kw), x, 0.0, 1.0, tol, tol)
                img = default_ops.quantize_u8(traj.contiguous())
            return mdist.all_gather_batch(img, B)

    return gen_1_img


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_channel", type=int, default=128)
    ap.add_argument("--input_dir", default="./results")
    ap.add_argument("--model", default="otcfm")
    ap.add_argument("--integration_steps", type=int, default=100)
    ap.add_argument("--integration_method", default="dopri5")
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--step", type=int, default=400000)
    ap.add_argument("--num_gen", type=int, default=50000)
    ap.add_argument("--batch_size_fid", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0, help="x0 stream seed, shared by all ranks (each takes its batch slice)")
    ap.add_argument("--guidance_scale", type=float, default=None, help="classifier-free guidance scale w (needs --num_classes); unset: unguided")
    ap.add_argument("--null_label", type=int, default=None, help="the class index trained as the null token (default: the last class)")
    ap.add_argument("--num_classes", type=int, default=None, help="build the class-conditional net (K + 1 classes with a null token); the checkpoint must be that net's")
    ap.add_argument("--cache_interval", type=int, default=None, help="feature reuse (DeepCache), euler only: one full U-Net evaluation in N steps; unset: every step is full")
    ap.add_argument("--cache_branch", type=int, default=None, help="feature reuse: the outermost block pairs recomputed at every step (default 1; UNetEngine.cache_branches() lists them)")
    a = ap.parse_args(argv)
    rank, world, local = mdist.init_from_env()
    device = f"cuda:{local}"
    net = build_model(a.num_channel, device, num_classes=a.num_classes)
    path = f"{a.input_dir}/{a.model}/{a.model}_cifar10_weights_step_{a.step}.pt"
    print("path: ", path)
    load_checkpoint(net, path)
    gen = make_gen_1_img(net, a.batch_size_fid, a.integration_steps, a.integration_method, device, a.tol, a.seed, a.guidance_scale, a.null_label,
                         a.cache_interval, a.cache_branch)
    try:
        from cleanfid import fid
    except ImportError as e:
        raise SystemExit("cleanfid is not installed (it downloads Inception weights and CIFAR statistics); "
                         "gen_1_img is ready for fid.compute_fid(gen=gen_1_img, ...) when it is") from e
    score = fid.compute_fid(gen=gen, dataset_name="cifar10", batch_size=a.batch_size_fid, dataset_res=32, num_gen=a.num_gen,
                            dataset_split="train", mode="legacy_tensorflow")
    if rank == 0:
        print("FID: ", score)


if __name__ == "__main__":
    main()
