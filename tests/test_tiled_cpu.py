"""CPU: tiled sampling (MultiDiffusion) - the library's host geometry (mi355_tile_count / mi355_tile_origins) against the restatement
(tests/tiled_ref.py), coverage and positive denominators, the refusals that need no handle, the restatement's own identity (one window is the
untiled sampler) and its discrimination: how far the plausible wrong implementations are from the right one, which is what makes the GPU
tolerances of tests/test_gpu_tiled.py meaningful.

The workspace rule and the refusals that read the handle (chunk above its largest batch, a short workspace, cond_drift) need a handle, and a
handle needs a device: they are in tests/test_gpu_tiled.py.
"""
import ctypes as C

import pytest
import torch

from mi355.synth import randn
from oracle import cfm_ref, unet_ref
from tests import tiled_ref as R
from tests.test_feature_cache_cpu import TINY, tiny_sd

AXES = [(16, 16, 8), (24, 16, 8), (40, 16, 8), (24, 16, 5), (40, 16, 7), (17, 16, 1), (32, 16, 16)]   # (L, S, s)


def _plan(Hc, Wc, sy, sx, weight=0, chunk=1):
    from mi355 import _lib

    return _lib.TilePlanC(Hc, Wc, sy, sx, weight, chunk)


def _count(S, plan):
    from mi355 import _lib

    out = (C.c_int32 * 3)()
    rc = _lib.lib().mi355_tile_count(S, C.byref(plan), out)
    return rc, list(out), _lib.lib().mi355_last_error().decode()


@pytest.mark.parametrize("L,S,s", AXES)
def test_geometry_against_restatement(L, S, s):
    from mi355 import _lib
    from mi355.engine import tile_plan

    want = R.axis_origins(L, S, s)
    if (L, S, s) == (24, 16, 5):
        assert want == [0, 5, 8]
    if (L, S, s) == (40, 16, 7):
        assert want == [0, 7, 14, 21, 24]
    if (L, S, s) == (16, 16, 8):
        assert want == [0]
    # the axis as the canvas height against another axis as its width, and the other way round
    for L2, S2, s2 in AXES:
        if S2 != S:
            continue
        want2 = R.axis_origins(L2, S, s2)
        plan = _plan(L, L2, s, s2)
        rc, out, _ = _count(S, plan)
        assert rc == 0 and out == [len(want), len(want2), len(want) * len(want2)]
        oy, ox = (C.c_int32 * out[0])(), (C.c_int32 * out[1])()
        assert _lib.lib().mi355_tile_origins(S, C.byref(plan), oy, ox) == 0
        assert list(oy) == want and list(ox) == want2
        tp = tile_plan(S, (L, L2), (s, s2))
        assert tp["origins"] == R.window_list((L, L2), S, (s, s2)) and tp["n_windows"] == out[2]
    # every pixel is covered, no window leaves the axis, and both weights give a positive denominator
    for weight in ("uniform", "tent"):
        den = torch.zeros(L, dtype=torch.float64)
        for o in want:
            assert 0 <= o <= L - S
            den[o:o + S] += R.taper(S, weight)
        assert bool((den > 0).all()), (L, S, s, weight)
    assert min(R.taper(S, "tent")) == 1 and max(R.taper(S, "tent")) == S // 2


def test_default_stride_and_python_plan():
    from mi355.engine import tile_plan

    tp = tile_plan(16, (24, 40))
    assert (tp["plan"].stride_y, tp["plan"].stride_x) == (8, 8) and (tp["ny"], tp["nx"], tp["n_windows"]) == (2, 4, 8)
    assert tp["oy"] == [0, 8] and tp["ox"] == [0, 8, 16, 24]
    with pytest.raises(ValueError, match="weight"):
        tile_plan(16, (24, 40), weight="gauss")


@pytest.mark.parametrize("plan,code,word", [
    ((15, 40, 8, 8, 0, 1), -2, "canvas_h"), ((24, 15, 8, 8, 0, 1), -2, "canvas_w"),
    ((24, 40, 0, 8, 0, 1), -1, "stride_y"), ((24, 40, 17, 8, 0, 1), -1, "stride_y"),
    ((24, 40, 8, 0, 0, 1), -1, "stride_x"), ((24, 40, 8, 17, 0, 1), -1, "stride_x"),
    ((24, 40, 8, 8, 2, 1), -1, "weight"), ((24, 40, 8, 8, -1, 1), -1, "weight"),
    ((24, 40, 8, 8, 0, 0), -1, "chunk"), ((24, 40, 8, 8, 0, -3), -1, "chunk"),
])
def test_refusals_without_a_handle(plan, code, word):
    from mi355 import _lib
    from mi355._lib import MI355BackendError
    from mi355.engine import tile_plan

    rc, _, msg = _count(16, _plan(*plan))
    assert rc == code and word in msg and msg.startswith("tile_count: "), (rc, msg)
    oy, ox = (C.c_int32 * 64)(), (C.c_int32 * 64)()
    assert _lib.lib().mi355_tile_origins(16, C.byref(_plan(*plan)), oy, ox) == code
    assert word in _lib.lib().mi355_last_error().decode()
    if word != "weight":
        with pytest.raises(MI355BackendError, match=word):
            tile_plan(16, plan[:2], plan[2:4], chunk=plan[5])
    # the op wrappers refuse the same plans before any launch (null pointers are never read)
    assert _lib.lib().mi355_tile_gather(None, None, 1, 3, 16, C.byref(_plan(*plan)), None) == code
    assert _lib.lib().mi355_tile_blend(None, None, None, 0.0, 1, 3, 16, C.byref(_plan(*plan)), None) == code


def test_null_plan_is_refused():
    from mi355 import _lib

    out = (C.c_int32 * 3)()
    assert _lib.lib().mi355_tile_count(16, None, out) == -1 and "plan" in _lib.lib().mi355_last_error().decode()


def test_one_window_is_the_untiled_sampler():
    """A canvas of the net's own size has one window with den = weight, and (weight * v) / weight is exact in fp64 for an fp32 v and these small
    integer weights: in the oracle's fp32 arithmetic the restatement IS oracle.cfm_ref.euler_trajectory, bit for bit, under both weights; its
    fp64 form (what the GPU loops are held to) stays within fp32 rounding of it."""
    sd, cfg = tiny_sd(0), TINY[0]
    x0 = randn(1, 2, 3, 16, 16)
    t = torch.full((2,), 0.25)
    for weight in ("uniform", "tent"):
        v = R.tiled_eval(sd, cfg, x0, 0.25, (8, 8), weight)
        assert torch.equal(v.float(), unet_ref.unet_forward(sd, cfg, x0, t))
    assert torch.equal(R.net_forward(sd, cfg, x0, t), unet_ref.unet_forward(sd, cfg, x0, t))
    ts = torch.linspace(0, 1, 5)
    want = cfm_ref.euler_trajectory(unet_ref.model_fn(sd, cfg), x0, ts)
    for weight in ("uniform", "tent"):
        assert torch.equal(R.tiled_euler(sd, cfg, x0, ts, (8, 8), weight, dtype=torch.float32), want)
    traj = R.tiled_euler(sd, cfg, x0, ts, (8, 8), "uniform")
    torch.testing.assert_close(traj.float(), want, rtol=1e-5, atol=1e-6)
    # cut is slicing, in batch order
    c = randn(2, 2, 3, 24, 40)
    w = R.cut(c, 16, (5, 7))
    wl = R.window_list((24, 40), 16, (5, 7))
    assert w.shape == (2 * 15, 3, 16, 16) and len(wl) == 15
    assert torch.equal(w[15 + 7], c[1, :, wl[7][0]:wl[7][0] + 16, wl[7][1]:wl[7][1] + 16])
    # blend_fp32 is blend in fp32
    v = randn(3, 30, 3, 16, 16)
    plan = dict(canvas_hw=(24, 40), stride=(5, 7), weight="tent")
    torch.testing.assert_close(R.blend_fp32(v, plan).double(), R.blend(v.double(), (24, 40), (5, 7), "tent"), rtol=1e-5, atol=1e-6)


def test_discrimination():
    """How far the plausible wrong tilings land from the right one after four Euler steps: last-window-wins instead of the average, the other
    weight, a stride without overlap, another overlapping stride.  Each is far outside the GPU tolerances (5e-4 relative in fp32, 0.08 absolute
    in bf16).  Probed before this test was written: 0.68, 0.55, 0.69, 0.75 at an output scale of 3.7."""
    sd, cfg = tiny_sd(0), TINY[0]
    x0 = randn(11, 2, 3, 24, 40)
    ts = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])
    base = R.tiled_euler(sd, cfg, x0, ts, (8, 8), "uniform")[-1]
    alts = {
        "last-window-wins": R.tiled_euler(sd, cfg, x0, ts, (8, 8), "uniform", last_wins=True)[-1],
        "tent weight": R.tiled_euler(sd, cfg, x0, ts, (8, 8), "tent")[-1],
        "stride (16, 16)": R.tiled_euler(sd, cfg, x0, ts, (16, 16), "uniform")[-1],
        "stride (5, 7)": R.tiled_euler(sd, cfg, x0, ts, (5, 7), "uniform")[-1],
    }
    print(f"baseline: stride (8, 8), uniform; output scale {float(base.abs().max()):.2f}")
    for name, v in alts.items():
        d = float((v - base).abs().max())
        print(f"   {name}: differs by {d:.2f}")
        assert d > 0.1, name


def test_python_refusals_before_any_device_work():
    from image_diffusion import sampling
    from image_diffusion.conditioning import ClassifierFreeGuidance, ReconstructionGuidance, Replacement
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM
    from torchcfm_compat import NeuralODE

    t = sampling.Tiling(stride=8, weight="tent", chunk=4)
    assert (t.stride, t.weight, t.chunk) == (8, "tent", 4)
    with pytest.raises(ValueError, match="weight"):
        sampling.Tiling(weight="gauss")
    with pytest.raises(ValueError, match="chunk"):
        sampling.Tiling(chunk=0)
    ddpm, lik = DDPM(5), InPainting(patch_size=6, pad_value=-2)
    eps = lambda x, t: x   # noqa: E731
    with pytest.raises(NotImplementedError, match="tiling.*ClassifierFreeGuidance"):
        sampling.get_conditional_sample_fn(eps, ddpm, ClassifierFreeGuidance(0.9, 0, 0.1, 2.0), lik, tiling=t)
    with pytest.raises(NotImplementedError, match="tiling.*ReconstructionGuidance"):
        sampling.get_conditional_sample_fn(eps, ddpm, ReconstructionGuidance(1.0, 1.0, "before", 0, 0.1), lik, tiling=t)
    with pytest.raises(NotImplementedError, match="tiling.*guided"):
        sampling.get_ddim_sample_fn(eps, ddpm.with_tiling(t), lik, guidance_scale=2.0)
    with pytest.raises(NotImplementedError, match="tiling.*multistep"):
        sampling.get_dpm_solver_sample_fn(eps, DDPM(25).with_tiling(t), lik)
    assert DDPM(100).with_tiling(t).respace(5).tiling is t and DDPM(25).tiling is None
    # an arbitrary callable sees whole frames only: tiling needs the fused loop
    with pytest.raises(NotImplementedError, match="tiling runs inside the fused loop"):
        sampling.get_prior_sample_fn(eps, ddpm, Replacement(0.1, 1.0, True, 0), lik, tiling=t)(torch.zeros(1, 3, 24, 24))
    with pytest.raises(NotImplementedError, match="tiling"):
        NeuralODE(lambda t, x: x, solver="euler", tiling=t)
    with pytest.raises(NotImplementedError, match="tiling"):
        NeuralODE(lambda t, x: x, solver="rk4", tiling=t)
