"""Digest of every sampler loop of libmi355_sampler.so on a tiny net with seeded inputs: one line per output tensor with its SHA-256, the
launch count mi355_unet_get_stats reports after the call, and the values of the workspace size functions.

The forward is bitwise reproducible (reductions run in a fixed order), so two builds of the library whose host code issues the same launches
with the same arguments print the same lines.  Run it once per library, each run in its own process:

    MI355_SAMPLER_LIB=/path/to/libmi355_sampler.so python tools/sampler_digest.py --out digest.txt [--save tensors.pt]

and compare the files.  --save keeps the tensors themselves, for a max-abs comparison of a case that is not reproducible run to run.
--mark launches one torch.flip kernel behind every case (nothing else here uses it), so that a kernel trace of the run
(rocprofv3 --kernel-trace -- python tools/sampler_digest.py --mark) can be cut into cases and compared case by case.

--cases forward adds (or, alone, selects) the digest of single forwards, on the smallest nets and batches at which each decision of the
executor (csrc/unet_engine.hip: unet_resolve) goes either way: per case the SHA-256 of the output, the launch count, every field of every
profile() record except ms, and for every conv output tensor whether read_tensor refuses it and why (0 readable, 1 never written, 2
normalised in place).  --cases hostloop: the Python samplers of image_diffusion/sampling.py on an untagged eps_model (the host loops over
the step ops), one line per (sampler, chain form, noise source), and ReconstructionGuidance in its three modes and both update rules.
--cases attention: one line per call of the three attention ops (qkv_attention, attn_block_fused, qkv_attention_vjp) on the shapes at which
each of the five attention kernels takes another path.  --inventory needs no GPU: the parameter inventory (names, shapes, order) and the
weight-image bytes of the same nets.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "image-inpainting-and-super-resolution-using-diffusion-models-and-conditional-flow-matching_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from image_diffusion.sde_diffusion import DDPM  # noqa: E402
from image_diffusion.unet import UNetModel, param_shapes  # noqa: E402
from mi355 import _lib  # noqa: E402
from mi355.engine import _PREC, MI355BackendError, param_inventory, tile_plan  # noqa: E402
from mi355.synth import randn, synth_state_dict  # noqa: E402

DEV = "cuda:0"
B, S, NS = 3, 16, 24   # batch, image size, DDPM steps (DDPM(Ns <= 20) has non-finite tables, as the reference does)
CANVAS, TILING = (24, 24), dict(stride=8, weight="uniform", chunk=5)   # tiled calls: 2 x 2 windows per canvas, B * 4 = 12 windows in chunks of 5
LINES, KEPT, MARK = [], {}, [False]


def net(prec, in_ch=3, num_classes=None, seed=0, out_ch=3, **debug):
    """The 16x16 / 32-channel two-level net of smoke(), with 3 output channels (out_ch=6: a learned-variance net of 3-channel states)."""
    kw = dict(image_size=S, in_channels=in_ch, model_channels=32, out_channels=out_ch, num_res_blocks=1, attention_resolutions=(2,),
              channel_mult=(1, 2), num_heads=2, num_classes=num_classes, precision=prec)
    m = UNetModel(**kw)
    m.load_state_dict(synth_state_dict(param_shapes(UNetModel(**kw)), 7000 + seed))
    if debug:
        m.debug = _lib.debug_config(**debug)
    return m.to(DEV).engine(DEV)


def emit(line):
    LINES.append(line)
    print(line, flush=True)


def case(prec, name, eng, outs):
    """outs: name -> tensor or None, the outputs of one sampler call on `eng`."""
    torch.cuda.synchronize()
    eng.check()
    launches = eng.stats(B)["launches"]
    if MARK[0]:
        torch.arange(4, device=DEV).flip(0)
    for k, t in outs.items():
        if t is None:
            continue
        t = t.detach().cpu().contiguous()
        KEPT[f"{prec}/{name}/{k}"] = t
        emit(f"{prec} {name} {k} {tuple(t.shape)} sha256={hashlib.sha256(t.numpy().tobytes()).hexdigest()} launches={launches}")


def sizes(prec, tag, eng):
    L = eng.L
    plan = tile_plan(S, CANVAS, TILING["stride"], TILING["weight"], TILING["chunk"])["plan"]
    for b in (1, B, 2 * B):
        emit(f"{prec} bytes {tag} ddpm_vlb_workspace batch={b} {L.mi355_ddpm_vlb_workspace_bytes(eng.handle, b)}")
        emit(f"{prec} bytes {tag} tiled_workspace batch={b} canvas={CANVAS} {L.mi355_tiled_workspace_bytes(eng.handle, b, C.byref(plan))}")
        for drift in (0, 1):
            emit(f"{prec} bytes {tag} feature_cache_workspace batch={b} branch=1 drift={drift} "
                 f"{L.mi355_feature_cache_workspace_bytes(eng.handle, b, 1, drift)}")
        emit(f"{prec} bytes {tag} unet_workspace batch={b} {L.mi355_unet_workspace_bytes(eng.handle, b)}")
        emit(f"{prec} bytes {tag} ddpm_cfg_workspace batch={b} {L.mi355_ddpm_cfg_workspace_bytes(eng.handle, b)}")
        for st in (1, 2, 3, 4):
            emit(f"{prec} bytes {tag} cfm_rk_workspace batch={b} stages={st} {L.mi355_cfm_rk_workspace_bytes(eng.handle, b, st)}")
            emit(f"{prec} bytes {tag} cfg_workspace batch={b} stages={st} {L.mi355_cfg_workspace_bytes(eng.handle, b, st)}")
        for g in (0, 1):
            emit(f"{prec} bytes {tag} ddpm_multistep_workspace batch={b} guided={g} {L.mi355_ddpm_multistep_workspace_bytes(eng.handle, b, g)}")
            for ms in (0, 1):
                emit(f"{prec} bytes {tag} ddpm_shaped_workspace batch={b} guided={g} multistep={ms} {L.mi355_ddpm_shaped_workspace_bytes(eng.handle, b, g, ms)}")
                emit(f"{prec} bytes {tag} ddpm_lv_workspace batch={b} guided={g} multistep={ms} {L.mi355_ddpm_lv_workspace_bytes(eng.handle, b, g, ms)}")
                emit(f"{prec} bytes {tag} ddpm_pred_workspace batch={b} guided={g} multistep={ms} {L.mi355_ddpm_pred_workspace_bytes(eng.handle, b, g, ms)}")
            for order in (2, 3, 4):
                for st in (1, 2, 4):
                    emit(f"{prec} bytes {tag} cfm_ab_workspace batch={b} order={order} start_stages={st} guided={g} "
                         f"{L.mi355_cfm_ab_workspace_bytes(eng.handle, b, order, st, g)}")
        for hl in (0, 4):
            emit(f"{prec} bytes {tag} cfm_recon_workspace batch={b} low={hl} {L.mi355_cfm_recon_workspace_bytes(eng.handle, b, hl, hl)}")


def span(n):
    return torch.linspace(0, 1, n + 1).tolist()


def sliced(eng, mb, fn):
    eng.max_batch_override = mb
    try:
        return fn()
    finally:
        eng.max_batch_override = None


def run(prec):
    u3, u6, l3, l6 = net(prec), net(prec, 6, seed=1), net(prec, 3, 10, seed=2), net(prec, 6, 4, seed=3)
    score = net(prec, seed=4)
    w3, w6 = net(prec, seed=5, out_ch=6), net(prec, 6, seed=6, out_ch=6)   # learned-variance nets: eps | v
    for tag, e in (("u3", u3), ("u6", u6), ("l3", l3), ("l6", l6), ("w3", w3), ("w6", w6)):
        sizes(prec, tag, e)
    x0 = randn(7101, B, 3, S, S).to(DEV)
    cond = (randn(7102, B, 3, S, S) * 0.5).clamp(-1, 1).to(DEV)
    cond[:, :, 4:10, 5:11] = -2.0
    y = torch.tensor([3, 0, 8], device=DEV)
    y4 = torch.tensor([2, 0, 1], device=DEV)
    wv = torch.tensor([0.5, 2.0, 3.5], device=DEV)
    xtu = ("x", "traj", "u8")

    # ---- flow-matching Euler ----
    case(prec, "euler_plain", u3, dict(zip(xtu, u3.cfm_euler(x0.clone(), span(3), keep_traj=True, want_u8=True))))
    case(prec, "euler_labels", l3, dict(zip(xtu, l3.cfm_euler(x0.clone(), span(3), keep_traj=True, want_u8=True, y=y))))
    case(prec, "euler_cond_drift", u6, dict(zip(xtu, u6.cfm_euler(x0.clone(), span(3), cond=cond, keep_traj=True, want_u8=True, cond_drift=True))))
    g3 = net(prec, sampler_graph=1)
    for rep in range(2):   # the recording call, then a replay
        case(prec, f"euler_graph_call{rep}", g3, dict(zip(xtu, g3.cfm_euler(x0.clone(), span(3), want_u8=True))))
    case(prec, "euler_sliced", u6, dict(zip(xtu, sliced(u6, 2, lambda: u6.cfm_euler(x0.clone(), span(3), cond=cond, keep_traj=True, want_u8=True)))))

    # ---- fixed-step Runge-Kutta: embedding table rows, and beyond EMB_TABLE_STEPS = 1024 rows one row set per evaluation ----
    for method, n_over in (("midpoint", 513), ("rk4", 257)):
        case(prec, f"rk_{method}_table", u3, dict(zip(xtu, u3.cfm_rk(x0.clone(), span(3), method, keep_traj=True, want_u8=True))))
        case(prec, f"rk_{method}_per_eval", u3, dict(zip(xtu, u3.cfm_rk(x0.clone(), span(n_over), method, want_u8=True))))
    case(prec, "rk_rk4_cond_table", u6, dict(zip(xtu, u6.cfm_rk(x0.clone(), span(3), "rk4", cond=cond, keep_traj=True, want_u8=True))))
    case(prec, "rk_rk4_labels_table", l3, dict(zip(xtu, l3.cfm_rk(x0.clone(), span(3), "rk4", keep_traj=True, want_u8=True, y=y))))
    case(prec, "rk_rk4_labels_per_eval", l3, dict(zip(xtu, l3.cfm_rk(x0.clone(), span(26), "rk4", want_u8=True, y=y))))   # 26 * 4 * 10 rows
    case(prec, "rk_one_time", u3, dict(zip(xtu, u3.cfm_rk(x0.clone(), [0.5], "rk4", keep_traj=True, want_u8=True))))
    case(prec, "rk_sliced", l3, dict(zip(xtu, sliced(l3, 2, lambda: l3.cfm_rk(x0.clone(), span(3), "heun2", keep_traj=True, want_u8=True, y=y)))))

    # ---- classifier-free guidance of the flow-matching samplers ----
    for wname, w in (("scalar", 2.0), ("per_image", wv)):
        case(prec, f"cfg_euler_labels_{wname}", l3,
             dict(zip(xtu, l3.cfm_euler(x0.clone(), span(3), keep_traj=True, want_u8=True, y=y, guidance_scale=w, null_label=9))))
        case(prec, f"cfg_rk4_labels_{wname}", l3,
             dict(zip(xtu, l3.cfm_rk(x0.clone(), span(3), "rk4", keep_traj=True, want_u8=True, y=y, guidance_scale=w, null_label=9))))
        case(prec, f"cfg_rk4_cond_{wname}", u6,
             dict(zip(xtu, u6.cfm_rk(x0.clone(), span(3), "rk4", cond=cond, keep_traj=True, want_u8=True, guidance_scale=w))))
    case(prec, "cfg_rk4_labels_cond", l6,
         dict(zip(xtu, l6.cfm_rk(x0.clone(), span(3), "rk4", cond=cond, keep_traj=True, want_u8=True, y=y4, guidance_scale=2.0, null_label=3))))
    case(prec, "cfg_rk4_labels_per_eval", l3, dict(zip(xtu, l3.cfm_rk(x0.clone(), span(26), "rk4", want_u8=True, y=y, guidance_scale=2.0, null_label=9))))
    case(prec, "cfg_one_time", l3, dict(zip(xtu, l3.cfm_rk(x0.clone(), [0.5], "rk4", keep_traj=True, want_u8=True, y=y, guidance_scale=2.0))))
    case(prec, "cfg_sliced", l3,
         dict(zip(xtu, sliced(l3, 2, lambda: l3.cfm_rk(x0.clone(), span(3), "midpoint", keep_traj=True, want_u8=True, y=y, guidance_scale=wv, null_label=9)))))

    # ---- DDPM / DDIM reverse loops: injected noise and device Philox noise ----
    ddpm = DDPM(NS)
    T = ddpm.host_tables()
    xT = randn(7201, B, 3, S, S).to(DEV)
    draws = torch.stack([randn(7210 + j, B, 3, S, S) for j in range(3 * NS)]).to(DEV)
    kw = dict(tmin=ddpm.tmin, tmax=ddpm.tmax)
    for nname, noise in (("injected", draws), ("philox", None)):
        kn = dict(kw, noise=noise, seed=1234)
        case(prec, f"ddpm_prior_{nname}", u3, {"x": u3.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_PRIOR, **kn)})
        case(prec, f"ddpm_replacement_{nname}", u3, {"x": u3.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_REPLACEMENT, cond=cond, **kn)})
        case(prec, f"ddpm_amortized_corr1_{nname}", u6, {"x": u6.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1, **kn)})
        case(prec, f"ddpm_ddim_{nname}", u6, {"x": u6.ddpm_sample(xT.clone(), T, mode=_lib.DDIM, cond=cond, **kn)})
        case(prec, f"ddpm_cfg_amortized_corr1_{nname}", u6,
             {"x": u6.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1, guidance_scale=2.0, **kn)})
        case(prec, f"ddpm_cfg_amortized_{nname}", u6, {"x": u6.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_AMORTIZED, cond=cond, guidance_scale=wv, **kn)})
        case(prec, f"ddpm_cfg_ddim_{nname}", u6, {"x": u6.ddpm_sample(xT.clone(), T, mode=_lib.DDIM, cond=cond, guidance_scale=2.0, **kn)})
        case(prec, f"ddpm_cfg_labels_cond_corr1_{nname}", l6,
             {"x": l6.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1, guidance_scale=2.0, y=y4, null_label=3, **kn)})
        case(prec, f"ddpm_cfg_sliced_{nname}", u6,
             {"x": sliced(u6, 2, lambda: u6.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1, guidance_scale=2.0, **kn))})

    # beyond the embedding table: Ns > 1024 steps, and Ns * num_classes > 1024 rows on the guided labelled path
    big, big_l = DDPM(1030), DDPM(260)
    case(prec, "ddpm_prior_per_eval", u3, {"x": u3.ddpm_sample(xT.clone(), big.host_tables(), mode=_lib.DDPM_PRIOR, tmin=big.tmin, tmax=big.tmax, seed=1234)})
    case(prec, "ddpm_cfg_labels_cond_per_eval", l6,
         {"x": l6.ddpm_sample(xT.clone(), big_l.host_tables(), mode=_lib.DDPM_AMORTIZED, cond=cond, guidance_scale=2.0, y=y4, null_label=3,
                              tmin=big_l.tmin, tmax=big_l.tmax, seed=1234)})

    # ---- the DDPM loops on a sub-sequence of the steps: respacing, DDIM(eta), a RePaint walk, DPM-Solver++, per-image shaping ----
    from image_diffusion.conditioning import repaint_walk
    r = ddpm.respace(8)
    R = r.host_tables()
    sched = dict(timesteps=r.timesteps, train_steps=r.base_Ns)
    rkw = dict(tmin=r.tmin, tmax=r.tmax, seed=1234)
    coefs = r.dpm_solver_coefs(2)
    walk = repaint_walk(r.Ns, 2, 2)
    assert any(b > a for a, b in zip(walk, walk[1:]))
    shaping = (0.9, 0.0, 0.7)   # quantile, no cap, rescale_phi (guided calls only: the rescale compares the guided eps with the conditional one)
    case(prec, "ddpm_respaced_prior", u3, {"x": u3.ddpm_sample(xT.clone(), R, mode=_lib.DDPM_PRIOR, noise=draws, **sched, **rkw)})
    case(prec, "ddpm_respaced_amortized_corr1", u6, {"x": u6.ddpm_sample(xT.clone(), R, mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1, **sched, **rkw)})
    for nname, noise in (("injected", draws), ("philox", None)):
        case(prec, f"ddpm_ddim_eta_{nname}", u6,
             {"x": u6.ddpm_sample(xT.clone(), R, mode=_lib.DDIM, cond=cond, noise=noise, ddim_sigma=r.ddim_sigma(0.5), **sched, **rkw)})
        case(prec, f"ddpm_cfg_ddim_eta_{nname}", u6,
             {"x": u6.ddpm_sample(xT.clone(), R, mode=_lib.DDIM, cond=cond, noise=noise, ddim_sigma=r.ddim_sigma(0.5), guidance_scale=wv, **sched, **rkw)})
    case(prec, "ddpm_repaint_walk", u3,
         {"x": u3.ddpm_sample(xT.clone(), R, mode=_lib.DDPM_REPLACEMENT, cond=cond, noise=draws, start_fraction=0.8, walk=walk, **sched, **rkw)})
    case(prec, "dpmpp_plain", u3, {"x": u3.ddpm_multistep(xT.clone(), R, coefs, **sched)})
    case(prec, "dpmpp_unscheduled", u3, {"x": u3.ddpm_multistep(xT.clone(), T, ddpm.dpm_solver_coefs(2))})
    case(prec, "dpmpp_guided_labels_cond", l6, {"x": l6.ddpm_multistep(xT.clone(), R, coefs, cond=cond, guidance_scale=2.0, y=y4, null_label=3, **sched)})
    for gname, eng, gkw, sh in (("plain", u3, {}, (0.9, 0.0, 0.0)), ("guided", u6, dict(cond=cond, guidance_scale=wv), shaping)):
        mode = _lib.DDIM if gkw else _lib.DDPM_PRIOR
        case(prec, f"shaped_{gname}_scheduled", eng,
             {"x": eng.ddpm_shaped(xT.clone(), R, sh, mode=mode, noise=draws, ddim_sigma=r.ddim_sigma(0.5) if gkw else None, **gkw, **sched, **rkw)})
        case(prec, f"shaped_{gname}_multistep", eng, {"x": eng.ddpm_shaped(xT.clone(), R, sh, mode=_lib.DDIM, coefs=coefs, **gkw, **sched)})
        case(prec, f"shaped_{gname}_none", eng, {"x": eng.ddpm_shaped(xT.clone(), R, None, mode=mode, noise=draws, **gkw, **sched, **rkw)})
    case(prec, "shaped_guided_amortized_corr1", u6,
         {"x": u6.ddpm_shaped(xT.clone(), T, shaping, mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1, guidance_scale=2.0, **kw, seed=1234)})
    case(prec, "ddpm_cfg_sliced_at_cfg_batch", u6,   # max_batch 4: cfg_batch() = 2, slices of 2 + 1 images
         {"x": sliced(u6, 4, lambda: u6.ddpm_sample(xT.clone(), R, mode=_lib.DDIM, cond=cond, guidance_scale=wv, ddim_sigma=r.ddim_sigma(0.5), **sched, **rkw))})
    case(prec, "shaped_guided_sliced", u6,
         {"x": sliced(u6, 4, lambda: u6.ddpm_shaped(xT.clone(), R, shaping, mode=_lib.DDIM, coefs=coefs, cond=cond, guidance_scale=wv, **sched))})

    # ---- Adams-Bashforth: a span that stays inside the start method (2 steps at order 3), and one that leaves it ----
    for n_steps in (2, 5):
        case(prec, f"ab3_plain_{n_steps}", u3, dict(zip(xtu, u3.cfm_ab(x0.clone(), span(n_steps), "ab3", keep_traj=True, want_u8=True))))
        case(prec, f"ab3_guided_{n_steps}", l6,
             dict(zip(xtu, l6.cfm_ab(x0.clone(), span(n_steps), "ab3", cond=cond, keep_traj=True, want_u8=True, y=y4, guidance_scale=wv, null_label=3))))
    case(prec, "ab2_one_time", u3, dict(zip(xtu, u3.cfm_ab(x0.clone(), [0.5], "ab2", keep_traj=True, want_u8=True))))

    # ---- training-free reconstruction: painting with replacement; low resolution with guidance and its loss ----
    xtul = ("x", "traj", "u8", "loss")
    case(prec, "recon_mode0_coupled", u3, dict(zip(xtul, u3.cfm_recon(x0.clone(), span(3), cond, 0, replace="coupled", final_paste=True, keep_traj=True, want_u8=True))))
    case(prec, "recon_mode0_fresh_philox", u3, dict(zip(xtul, u3.cfm_recon(x0.clone(), span(3), cond, 0, replace="fresh", seed=99, want_u8=True))))
    if prec == "fp32":   # (the differentiable plan is digested in fp32 only, as in run_forward)
        d3 = UNetModel(image_size=S, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
                       num_heads=2, precision=prec)
        d3.load_state_dict(synth_state_dict(param_shapes(d3), 7005))
        d3 = d3.to(DEV).engine(DEV, differentiable=True)
        ylow = (randn(7103, B, 3, 4, 4) * 0.5).to(DEV)
        case(prec, "recon_mode2_loss", d3, dict(zip(xtul, d3.cfm_recon(x0.clone(), span(3), ylow, 2, scales=[0.5, 0.0, 0.25], keep_traj=True, want_u8=True,
                                                                        return_loss=True))))

    # ---- SF2M Euler-Maruyama: two nets, two output times inside step 1 ----
    grid = span(3)
    dW = torch.stack([randn(7300 + j, B, 3, S, S) * 0.5 for j in range(3)]).to(DEV)
    outs = [(0, 0.0), (1, 0.25), (1, 0.75), (2, 1.0)]
    for rev in (False, True):
        for nname, nk in (("injected", dict(dW=dW)), ("philox", dict(seed=77))):
            case(prec, f"sf2m_{'reverse' if rev else 'forward'}_{nname}", u3,
                 dict(zip(("x", "traj"), u3.sf2m_euler(score, x0.clone(), grid, 0.3, reverse=rev, outputs=outs, **nk))))
    case(prec, "sf2m_per_eval", u3, {"x": u3.sf2m_euler(score, x0.clone(), span(1030), 0.3, seed=77)[0]})
    case(prec, "sf2m_sliced", u3, dict(zip(("x", "traj"), sliced(u3, 2, lambda: u3.sf2m_euler(score, x0.clone(), grid, 0.3, outputs=outs, seed=77)))))

    # ---- the slicing loops of the Adams-Bashforth and the reconstruction samplers ----
    case(prec, "ab3_plain_sliced", u3, dict(zip(xtu, sliced(u3, 2, lambda: u3.cfm_ab(x0.clone(), span(5), "ab3", keep_traj=True, want_u8=True)))))
    case(prec, "ab3_guided_sliced", l6, dict(zip(xtu, sliced(l6, 4, lambda: l6.cfm_ab(
        x0.clone(), span(5), "ab3", cond=cond, keep_traj=True, want_u8=True, y=y4, guidance_scale=wv, null_label=3)))))
    case(prec, "recon_mode0_fresh_philox_sliced", u3, dict(zip(xtul, sliced(u3, 2, lambda: u3.cfm_recon(
        x0.clone(), span(3), cond, 0, replace="fresh", seed=99, final_paste=True, keep_traj=True, want_u8=True)))))

    # ---- feature reuse across steps (DeepCache): Euler with an interval and with an explicit schedule and its drift; the DDPM loops ----
    xtud = ("x", "traj", "u8", "drift")
    full = [1, 0, 1, 1, 0, 0]
    case(prec, "euler_cached_interval", u3, dict(zip(xtu, u3.cfm_euler(x0.clone(), span(6), keep_traj=True, want_u8=True, cache_interval=3))))
    case(prec, "euler_cached_schedule_drift", l3,
         dict(zip(xtud, l3.cfm_euler(x0.clone(), span(6), keep_traj=True, want_u8=True, y=y, cache_schedule=full, cache_drift=True))))
    case(prec, "euler_cached_schedule_drift_sliced", l3, dict(zip(xtud, sliced(l3, 2, lambda: l3.cfm_euler(
        x0.clone(), span(6), keep_traj=True, want_u8=True, y=y, cache_schedule=full, cache_drift=True)))))
    case(prec, "ddpm_cached_unscheduled", u3, {"x": u3.ddpm_sample(xT.clone(), T, mode=_lib.DDPM_PRIOR, cache_interval=2, **kw, seed=1234)})
    case(prec, "ddpm_cached_respaced_corr1", u6,
         {"x": u6.ddpm_sample(xT.clone(), R, mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1, cache_interval=3, noise=draws, **sched, **rkw)})

    # ---- tiled calls: 24x24 canvases, windows of the net's 16x16 at stride 8, more than one chunk ----
    xc = randn(7401, B, 3, *CANVAS).to(DEV)
    cc = (randn(7402, B, 3, *CANVAS) * 0.5).clamp(-1, 1).to(DEV)
    xTc = randn(7403, B, 3, *CANVAS).to(DEV)
    case(prec, "forward_tiled", u3, {"out": u3.forward_tiled(xc, 0.3, tiling=TILING)})
    case(prec, "euler_tiled", u3, dict(zip(xtu, u3.cfm_euler(xc.clone(), span(3), keep_traj=True, want_u8=True, tiling=TILING))))
    case(prec, "euler_tiled_labels_cond", l6,
         dict(zip(xtu, l6.cfm_euler(xc.clone(), span(3), cond=cc, keep_traj=True, want_u8=True, y=y4, tiling=dict(TILING, weight="tent")))))
    case(prec, "ddpm_tiled_amortized_corr1", u6,
         {"x": u6.ddpm_sample(xTc.clone(), T, mode=_lib.DDPM_AMORTIZED, cond=cc, n_corrector=1, tiling=TILING, **kw, seed=1234)})
    case(prec, "ddpm_tiled_ddim_respaced", u3, {"x": u3.ddpm_sample(xTc.clone(), R, mode=_lib.DDIM, tiling=TILING, **sched, **rkw)})

    # ---- learned-variance nets (6 output channels: eps | v) ----
    ml = r.max_log()
    times = [r.time(k) for k in range(r.Ns)]
    case(prec, "learned_ancestral", w3, {"x": w3.ddpm_learned(xT.clone(), R, ml, mode=_lib.DDPM_PRIOR, noise=draws, **sched, **rkw)})
    case(prec, "learned_guided_sliced", w6, {"x": sliced(w6, 4, lambda: w6.ddpm_learned(
        xT.clone(), R, ml, mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1, guidance_scale=wv, **sched, **rkw))})
    case(prec, "learned_multistep", w3, {"x": w3.ddpm_learned(xT.clone(), R, ml, mode=_lib.DDIM, coefs=coefs, **sched)})
    case(prec, "learned_none_times", u3, {"x": u3.ddpm_learned(xT.clone(), R, None, mode=_lib.DDPM_PRIOR, times=times, **sched, **rkw)})

    # ---- x0- and v-prediction nets ----
    for kind in ("x0", "v"):
        case(prec, f"pred_{kind}_plain", u3, {"x": u3.ddpm_pred(xT.clone(), R, kind, mode=_lib.DDPM_PRIOR, noise=draws, **sched, **rkw)})
        case(prec, f"pred_{kind}_guided", u6,
             {"x": u6.ddpm_pred(xT.clone(), R, kind, mode=_lib.DDPM_AMORTIZED, cond=cond, n_corrector=1, guidance_scale=wv, **sched, **rkw)})
    case(prec, "pred_v_guided_shaped", u6,
         {"x": u6.ddpm_pred(xT.clone(), R, "v", mode=_lib.DDIM, shaping=shaping, cond=cond, guidance_scale=2.0, ddim_sigma=r.ddim_sigma(0.5), **sched, **rkw)})
    case(prec, "pred_x0_multistep", u3, {"x": u3.ddpm_pred(xT.clone(), R, "x0", mode=_lib.DDIM, coefs=coefs, **sched)})
    case(prec, "ddpm_sample_prediction_v", u3, {"x": u3.ddpm_sample(xT.clone(), R, mode=_lib.DDPM_PRIOR, prediction="v", **sched, **rkw)})

    # ---- the variational bound: every step of the respaced chain in one call ----
    ts_ = ("terms", "summary")
    xd = x0.clamp(-1, 1)
    vn = draws[:r.Ns].contiguous()
    fixed, learned = r.vlb_log_variances("fixed_small"), r.vlb_log_variances("learned")
    for nname, nk in (("injected", dict(noise=vn)), ("philox", dict(seed=55))):
        case(prec, f"vlb_fixed_{nname}", u3, dict(zip(ts_, u3.ddpm_vlb(xd, R, fixed, learned=False, **nk))))
        case(prec, f"vlb_learned_{nname}", w6, dict(zip(ts_, w6.ddpm_vlb(xd, R, learned, learned=True, cond=cond, times=times, **nk))))
    case(prec, "vlb_pred_x0", u3, dict(zip(ts_, u3.ddpm_vlb(xd, R, fixed, learned=False, prediction="x0", seed=55))))
    case(prec, "vlb_fixed_sliced", l3, dict(zip(ts_, sliced(l3, 2, lambda: l3.ddpm_vlb(xd, R, fixed, learned=False, y=y, cdf="tanh", seed=55)))))


# ---- the Python samplers' host loops (image_diffusion/sampling.py) on an untagged eps_model ----------------------------------------------
def run_hostloop(prec):
    """One line per (sampler, chain form, noise source): the result of sample() with an untagged `lambda xi, i: fast(xi, i)` around an
    engine-backed model - the host loop over the step ops - on a 4-step respacing; a refused pair (NotImplementedError, ValueError) prints the exception's type and message; any other
    exception ends the run.
    ReconstructionGuidance (three likelihoods, both update rules) takes the tagged model, as it must.  Every case starts from a fresh
    _draw_counter / _noise_offset and the same torch.manual_seed."""
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized, ClassifierFreeGuidance, NullSpace, ReconstructionGuidance, RePaint, Replacement
    from image_diffusion.likelihoods import AveragePooling, HyperResolution, InPainting, LowResolution
    from image_diffusion.sde_diffusion import linear_betas

    def model(in_ch, out_ch, seed):
        kw = dict(image_size=S, in_channels=in_ch, model_channels=32, out_channels=out_ch, num_res_blocks=1, attention_resolutions=(2,),
                  channel_mult=(1, 2), num_heads=2, precision=prec)
        m = UNetModel(**kw)
        m.load_state_dict(synth_state_dict(param_shapes(UNetModel(**kw)), 7000 + seed))
        return m.to(DEV)

    nets = {(3, 3): model(3, 3, 0), (6, 3): model(6, 3, 1), (3, 6): model(3, 6, 5), (6, 6): model(6, 6, 6)}
    base = DDPM(NS).respace(4)
    scaled = DDPM.from_betas(linear_betas(NS), time_scale=float(NS)).respace(4)
    chains = {
        "plain": base, "shaped_q": base.with_x0_shaping(dynamic_threshold=0.9),
        "shaped_q_rescale": base.with_x0_shaping(dynamic_threshold=0.9, guidance_rescale=0.7), "learned": base.with_learned_variance(),
        "x0": base.with_prediction("x0"), "v": base.with_prediction("v"), "v_learned": base.with_prediction("v").with_learned_variance(),
        "v_shaped": base.with_prediction("v").with_x0_shaping(dynamic_threshold=0.9), "time_scale": scaled,
    }
    xT = randn(7201, B, 3, S, S).to(DEV)
    cond = (randn(7102, B, 3, S, S) * 0.5).clamp(-1, 1).to(DEV)
    cond[:, :, 4:10, 5:11] = -2.0
    ylow = (randn(7103, B, 3, 4, 4) * 0.5).to(DEV)
    draws = [randn(7210 + j, B, 3, S, S).to(DEV) for j in range(40)]
    wv = torch.tensor([0.5, 2.0, 3.5], device=DEV)
    lik, pool = InPainting(patch_size=6, pad_value=-2.0), AveragePooling(4)
    cnd = lambda c, k, **kw: (lambda e, d: sampling.get_conditional_sample_fn(e, d, c, k, **kw))   # noqa: E731
    with_cond, alone = (lambda s: s(xT, cond)), (lambda s: s(xT))
    # name -> (net input channels, factory(eps_model, chain), call(sample))
    samplers = {
        "prior_unconditional": (3, lambda e, d: sampling.get_prior_sample_fn(e, d, Replacement(0.1, 1.0, True, 0), lik), alone),
        "prior_amortized": (6, lambda e, d: sampling.get_prior_sample_fn(e, d, Amortized(0.1, 0, 0.1), lik), alone),
        "amortized": (6, cnd(Amortized(0.1, 0, 0.1), lik), with_cond),
        "amortized_corrector": (6, cnd(Amortized(0.1, 1, 0.25), lik), with_cond),
        "replacement_noisy": (3, cnd(Replacement(0.1, 0.6, True, 0), lik), with_cond),
        "replacement_clean_corrector": (3, cnd(Replacement(0.2, 0.6, False, 1), lik), with_cond),
        "repaint_walk": (3, cnd(RePaint(0.1, 0.6, True, 0, 1, 2), lik), with_cond),
        "cfg_float_corrector": (6, cnd(ClassifierFreeGuidance(0.1, 1, 0.1, 2.0), lik), with_cond),
        "ddim_eta0": (3, lambda e, d: sampling.get_ddim_sample_fn(e, d, lik), alone),
        "ddim_eta05": (3, lambda e, d: sampling.get_ddim_sample_fn(e, d, None, eta=0.5), alone),
        "ddim_eta0_guided": (6, lambda e, d: sampling.get_ddim_sample_fn(e, d, lik, guidance_scale=2.0), with_cond),
        "ddim_eta05_guided_tensor_w": (6, lambda e, d: sampling.get_ddim_sample_fn(e, d, None, guidance_scale=wv, eta=0.5), with_cond),
        "dpm1": (3, lambda e, d: sampling.get_dpm_solver_sample_fn(e, d, None, order=1), alone),
        "dpm2_condition": (6, lambda e, d: sampling.get_dpm_solver_sample_fn(e, d, lik, order=2), with_cond),
        "dpm1_guided_likelihood": (6, lambda e, d: sampling.get_dpm_solver_sample_fn(e, d, lik, guidance_scale=2.0, order=1), with_cond),
        "dpm2_guided": (6, lambda e, d: sampling.get_dpm_solver_sample_fn(e, d, None, guidance_scale=wv, order=2), with_cond),
        "nullspace_ancestral": (3, cnd(NullSpace(0.0, None, 1, 1), lik), with_cond),
        "nullspace_ancestral_plus_walk": (3, cnd(NullSpace(0.3, None, 1, 2), lik), with_cond),
        "nullspace_ddim_eta0": (3, cnd(NullSpace(0.0, 0.0, 1, 1), lik), with_cond),
        "nullspace_ddim_eta05_walk_pool": (3, cnd(NullSpace(0.0, 0.5, 1, 2), pool), lambda s: s(xT, pool.sample(cond))),
    }
    recon = {}
    for rule in ("before", "after"):
        recon[f"recon_painting_{rule}"] = (cnd(ReconstructionGuidance(0.5, 0.6, rule, 1, 0.1), lik), with_cond)
        recon[f"recon_hyper_{rule}"] = (cnd(ReconstructionGuidance(0.5, 0.6, rule, 0, 0.1), HyperResolution(4, 4)), with_cond)
        recon[f"recon_lowres_{rule}"] = (cnd(ReconstructionGuidance(0.5, 0.6, rule, 0, 0.1), LowResolution(4, 4)), lambda s: s(xT, ylow))

    def one(name, cname, nname, factory, call, eps_model, chain):
        sampling._draw_counter, sampling._noise_offset = 0, 0
        torch.manual_seed(1234)
        try:
            sample = factory(eps_model, chain)
            if nname == "injected":
                with sampling.injected_noise(draws):
                    x = call(sample)
            else:
                x = call(sample)
        except (NotImplementedError, ValueError) as e:   # the refusals raised on purpose; anything else (the backend, the device) ends the run
            emit(f"{prec} hostloop {name} {cname} {nname} refused {type(e).__name__} {str(e)!r}")
            return
        torch.cuda.synchronize()
        if MARK[0]:
            torch.arange(4, device=DEV).flip(0)
        t = x.detach().cpu().contiguous()
        KEPT[f"{prec}/hostloop/{name}/{cname}/{nname}"] = t
        emit(f"{prec} hostloop {name} {cname} {nname} {tuple(t.shape)} sha256={hashlib.sha256(t.numpy().tobytes()).hexdigest()} "
             f"draws={sampling._draw_counter} offset={sampling._noise_offset}")

    for cname, chain in chains.items():
        out_ch = 6 if chain.learned_variance else 3
        for name, (in_ch, factory, call) in samplers.items():
            fast = sampling.make_eps_model(nets[(in_ch, out_ch)], chain)
            generic = lambda xi, i, fast=fast: fast(xi, i)   # noqa: E731  (untagged: the host loop over the step ops)
            for nname in ("injected", "philox"):
                one(name, cname, nname, factory, call, generic, chain)
    for name, (factory, call) in recon.items():   # (every other chain form is refused at the factory: the CPU transcripts hold those rows)
        for nname in ("injected", "philox"):
            one(name, "plain", nname, factory, call, sampling.make_eps_model(nets[(3, 3)], base), base)


# ---- single forwards --------------------------------------------------------------------------------------------------------------------
CIFAR = dict(image_size=32, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(2,),
             channel_mult=(1, 2, 2, 2), num_heads=4, num_head_channels=64)
TWO_LEVEL = dict(CIFAR, num_res_blocks=1, channel_mult=(1, 2))                       # 32 px / 128 channels: the edge convs' kernels
UPDOWN = dict(image_size=16, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=(2,),
              channel_mult=(1, 2, 2), num_heads=2, use_scale_shift_norm=True, resblock_updown=True)   # smallest with a down and an up ResBlock
TINY = dict(image_size=S, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
            num_heads=2)
FWD_NETS = {
    "cifar": CIFAR, "cifar_film": dict(CIFAR, use_scale_shift_norm=True), "cifar_in6": dict(CIFAR, in_channels=6),
    "two_level": TWO_LEVEL, "two_level_in6": dict(TWO_LEVEL, in_channels=6),
    "updown": UPDOWN, "updown_noconv": dict(UPDOWN, conv_resample=False),
    "plain_resample": dict(UPDOWN, resblock_updown=False, conv_resample=False),      # the parameter-free pool / nearest-x2 ops
    "classcond": dict(TINY, num_classes=10),
    "differentiable": UPDOWN,   # (its pool + affine and GroupNorm passes then run on per-site statistics)
}


def fwd_model(tag, prec, seed=0):
    m = UNetModel(precision=prec, **FWD_NETS[tag])
    m.load_state_dict(synth_state_dict(param_shapes(m), 7500 + seed))
    return m


def fwd_engine(tag, prec, differentiable=False, **debug):
    m = fwd_model(tag, prec)
    if debug:
        m.debug = _lib.debug_config(**debug)
    return m.to(DEV).engine(DEV, differentiable=differentiable)


def inventory():
    for tag in FWD_NETS:
        m = fwd_model(tag, "fp32")
        for prec in ("fp32", "bf16"):
            cfg = _lib.make_config(dtype=_PREC[prec], differentiable=tag == "differentiable", debug=None, **m._cfg_kwargs())
            inv = param_inventory(cfg)
            text = "\n".join(f"{n} {s}" for n, s in inv)
            emit(f"inventory {tag} {prec} params={len(inv)} sha256={hashlib.sha256(text.encode()).hexdigest()} "
                 f"weight_bytes={_lib.lib().mi355_unet_weight_bytes(cfg)}")
            KEPT[f"inventory/{tag}/{prec}"] = text


def fwd_case(prec, name, eng, b, cond=False, y=None, euler=False, vjp=False):
    """One forward at batch b (and its profile(), read_tensor verdicts; optionally a 4-step Euler loop / the vjp behind it)."""
    sz, cin = eng.image_size, eng.in_channels
    x = randn(7601, b, 3, sz, sz).to(DEV)
    c = (randn(7602, b, cin - 3, sz, sz) * 0.5).to(DEV) if cond else None
    t = torch.linspace(0.1, 0.9, b).to(DEV)
    out = eng.forward(x, t, cond=c, y=y)
    torch.cuda.synchronize()
    eng.check()
    launches = eng.stats(b)["launches"]
    outs = {"out": out}
    if vjp:
        outs["grad_x"] = eng.vjp(randn(7603, b, 3, sz, sz).to(DEV))
    verdicts = []
    for op in eng.plan_ops():
        if op["kind"] != 1 or op["dst"] < 0:
            continue
        try:
            eng.read_tensor(op["dst"], b, (op["dst_c"], op["dst_h"], op["dst_h"]))
            verdicts.append("0")
        except MI355BackendError as e:
            verdicts.append("1" if "did not materialise" in str(e) else "2" if "normalised this conv output in place" in str(e) else "?")
    recs = eng.profile(x, t, cond=c) if y is None else []   # (profile() has no labelled form)
    torch.cuda.synchronize()
    if MARK[0]:
        torch.arange(4, device=DEV).flip(0)
    for k, v in outs.items():
        v = v.detach().cpu().contiguous()
        KEPT[f"{prec}/{name}/{k}"] = v
        emit(f"{prec} {name} {k} {tuple(v.shape)} sha256={hashlib.sha256(v.numpy().tobytes()).hexdigest()} launches={launches}")
    emit(f"{prec} {name} read_tensor {''.join(verdicts)}")
    emit(f"{prec} {name} profile launches_after={eng.stats(b)['launches']} " + ";".join(
        f"{r['kind']}/{r['ks']}/{r['cin']}/{r['cout']}/{r['h']}x{r['w']}/{r['tile'][0]}x{r['tile'][1]}/{r['flops']!r}/{r['bytes']!r}" for r in recs))
    if euler:
        xs = eng.cfm_euler(x.clone(), span(4), cond=c, y=y)[0]
        torch.cuda.synchronize()
        eng.check()
        n = eng.stats(b)["launches"]
        if MARK[0]:
            torch.arange(4, device=DEV).flip(0)
        xs = xs.detach().cpu().contiguous()
        KEPT[f"{prec}/{name}/euler4"] = xs
        emit(f"{prec} {name} euler4 {tuple(xs.shape)} sha256={hashlib.sha256(xs.numpy().tobytes()).hexdigest()} launches={n}")


def run_forward(prec):
    pp = _lib.debug_config().conv_pp
    knobs = [("default", {}), ("gn_epilogue0", dict(gn_epilogue=0)), ("gn_epilogue1", dict(gn_epilogue=1)), ("gn_epilogue3", dict(gn_epilogue=3)),
             ("conv_small7", dict(conv_small=7)), ("gn_fuse0", dict(gn_fuse=0))]
    for kname, kw in knobs:
        e = fwd_engine("cifar", prec, **kw)
        for b in (8, 256):   # fewer tiles than CUs (generic tiles, K-sharing small-level forms) | persistent kernels, in-place 16x16 norm
            fwd_case(prec, f"fwd_cifar_{kname}_b{b}", e, b)
        del e
    for tag in ("two_level", "two_level_in6"):   # first conv reading NCHW, last conv applying the Euler step - and neither
        for edge in (15, 3):
            fwd_case(prec, f"fwd_{tag}_edge{edge}_b18", fwd_engine(tag, prec, conv_edge=edge), 18, cond=tag.endswith("in6"), euler=True)
    fwd_case(prec, "fwd_cifar_in6_b8", fwd_engine("cifar_in6", prec), 8, cond=True)
    for tag in ("updown", "updown_noconv", "plain_resample"):
        fwd_case(prec, f"fwd_{tag}_b3", fwd_engine(tag, prec), 3)
    cc = fwd_engine("classcond", prec)
    fwd_case(prec, "fwd_classcond_b3", cc, 3, y=torch.tensor([3, 0, 8], device=DEV), euler=True)   # per-forward rows, then table rows
    if prec == "bf16":
        e = fwd_engine("cifar_film", prec)
        for b in (8, 256):
            fwd_case(prec, f"fwd_cifar_film_b{b}", e, b)
        del e
        for bit in (1, 0):   # batch 64: the smallest where the phase-form upsample conv is eligible
            fwd_case(prec, f"fwd_cifar_pp_phase{bit}_b64", fwd_engine("cifar", prec, conv_pp=(pp | 64) if bit else (pp & ~64)), 64)
    if prec == "fp32":
        fwd_case(prec, "fwd_differentiable_b3", fwd_engine("differentiable", prec, differentiable=True), 3, vjp=True)


# ---- the attention ops, one call each ---------------------------------------------------------------------------------------------------
ATTN_SHAPES = [(2, 4, 64, 16), (2, 1, 64, 49), (1, 1, 192, 70), (1, 2, 128, 100), (2, 4, 64, 256), (2, 1, 96, 256), (1, 3, 32, 300), (1, 1, 256, 256),
               (2, 1, 384, 256), (2, 1, 512, 64)]   # (B, heads, ch, T): every launch_attn case, both QB, ragged last tiles, 32-key tiles, single-buffer fp32


def run_attention():
    """One line per call of ops.qkv_attention, ops.attn_block_fused and ops.qkv_attention_vjp, on the shapes the tests name as the smallest at
    which each kernel path can go wrong; fixed-seed inputs, both channel orders, every precision the op accepts."""
    from mi355.ops import default_ops as ops

    names = {_lib.MI355_F32: "fp32", _lib.MI355_BF16: "bf16", _lib.MI355_F16: "fp16"}
    orders = ((False, "legacy"), (True, "new"))

    def line(tag, t):
        torch.cuda.synchronize()
        t = t.detach().cpu().contiguous()
        KEPT[f"attention/{tag}"] = t
        emit(f"attention {tag} {tuple(t.shape)} sha256={hashlib.sha256(t.numpy().tobytes()).hexdigest()}")

    # the generic kernel
    for i, (b, heads, ch, t) in enumerate(ATTN_SHAPES):
        qkv = (randn(7700 + i, b, 3 * heads * ch, t) * 0.5).to(DEV)
        for new, oname in orders:
            for dt, dname in names.items():
                line(f"qkv {dname} {oname} B{b} H{heads} ch{ch} T{t}", ops.qkv_attention(qkv, heads, new, dt))
    # its softmax slow path: a late huge key, and every logit near -288 (tests/test_gpu_ops.py: test_attention_softmax_spike)
    ch, t = 64, 256
    late = randn(11, 1, 3 * ch, t) * 0.5
    late[0, ch:2 * ch, 200] = late[0, 0:ch, 7] * 40.0
    low = randn(12, 1, 3 * ch, t) * 0.5
    low[0, 0:ch] = 6.0 + 0.1 * low[0, 0:ch]
    low[0, ch:2 * ch] = -6.0 + 0.1 * low[0, ch:2 * ch]
    for sname, q in (("late_key", late), ("all_low", low)):
        for dt, dname in names.items():
            line(f"qkv_spike {sname} {dname}", ops.qkv_attention(q.to(DEV), 1, False, dt))

    # the fused block: per-image kernel (knob 3), then the persistent kernel through the knob's lane override
    def block(seed, n, c, t):
        return ((randn(seed, n, c, t)).to(DEV), (1.0 + 0.2 * randn(seed + 1, n, c)).to(DEV), (0.2 * randn(seed + 2, n, c)).to(DEV),
                randn(seed + 3, 3 * c, c) / c ** 0.5, 0.1 * randn(seed + 4, 3 * c))

    for t in (128, 256):
        for c in (128, 256, 384, 512):
            for n in (1, 9):
                x, a, b, w, bias = block(7800 + t + c + 7 * n, n, c, t)
                for new, oname in orders:
                    for dt, dname in names.items():
                        out, form = ops.attn_block_fused(x, a, b, w, bias, c // 64, new, dt, debug=_lib.debug_config(attn_fused=3))
                        line(f"fused_image {dname} {oname} T{t} C{c} N{n} form={form}", out)
    for c in (128, 256):
        for n, lanes in ((24, 5), (3, 8), (17, 8)):
            x, a, b, w, bias = block(7900 + c + 7 * n, n, c, 256)
            for new, oname in orders:
                for dt in (_lib.MI355_BF16, _lib.MI355_F16):
                    out, form = ops.attn_block_fused(x, a, b, w, bias, c // 64, new, dt, debug=_lib.debug_config(attn_fused=1 | (lanes << 8)))
                    line(f"fused_persistent {names[dt]} {oname} C{c} N{n} lanes{lanes} form={form}", out)

    # the backward
    for ch in (32, 64, 96, 128, 192, 256):
        for t in (70, 256):
            heads = 2 if ch <= 64 else 1
            qkv = (randn(8000 + ch + t, 2, 3 * heads * ch, t) * 0.5).to(DEV)
            g = randn(8001 + ch + t, 2, heads * ch, t).to(DEV)
            for new, oname in orders:
                for dt in (_lib.MI355_F32, _lib.MI355_BF16):
                    line(f"qkv_vjp {names[dt]} {oname} H{heads} ch{ch} T{t}", ops.qkv_attention_vjp(qkv, g, heads, new, dt))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--save", help="keep every output tensor in this torch file")
    ap.add_argument("--mark", action="store_true", help="one torch.flip launch behind every case: the cut marks of a kernel trace")
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--cases", default="sampler", help="comma list of: sampler (the loops), forward (single forwards), hostloop (the Python samplers on an untagged eps_model), "
                    "attention (the attention ops; once, not per precision)")
    ap.add_argument("--inventory", action="store_true", help="no GPU: parameter inventories and weight-image bytes of the forward nets only")
    a = ap.parse_args()
    MARK[0] = a.mark
    emit(f"mi355_version {_lib.lib().mi355_version()}")
    if a.inventory:
        inventory()
    for prec in () if a.inventory else a.precisions.split(","):
        if "sampler" in a.cases.split(","):
            run(prec)
        if "forward" in a.cases.split(","):
            run_forward(prec)
        if "hostloop" in a.cases.split(","):
            run_hostloop(prec)
    if not a.inventory and "attention" in a.cases.split(","):
        run_attention()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    if a.save:
        torch.save(KEPT, a.save)


if __name__ == "__main__":
    main()
