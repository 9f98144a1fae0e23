"""GPU: the fixed-step explicit Runge-Kutta CFM samplers (midpoint, Heun, RK4, the 3/8 rule) on the HIP path.

- the stage op (mi355_rk_stage) against fp64: vector and scalar paths, in place, its fused copy and uint8 outputs, guards;
- the one-call sampler (mi355_cfm_rk_sample, UNetEngine.cfm_rk) in fp32 against tests.test_rk_cpu.fixed_rk_ref, the textbook restatement
  over the oracle's U-Net: unconditional, with labels, with a condition, in slices, past the embedding table, bf16;
- Euler through the tableau against the Euler sampler, NeuralODE's one-call fast path against the host-driven FixedStepRK loop,
  compute_fid's --integration_method, and the library's refusals.

Tolerances: fp32 the CFM bound of test_gpu_configs.py (rtol 5e-4, atol 1e-4); bf16 its 3-step bounds (max 3 % of scale, rms 1 %); the
fast path against the host loop rtol 1e-4 / atol 1e-4 (test_gpu_sde.test_fast_path_vs_host_driven_notebook_class).
Stage op: |got - fp64| <= (nk + 1) * eps32 * (|y0| + sum_j |c_j k_j|) elementwise - at most 2 nk + 1 roundings (nk products, nk partial sums,
the final sum), each at most half an ulp (eps32 / 2 relative) of a value bounded by that magnitude, whether or not a product and its sum
are contracted to one fma.
"""
import ctypes as C

import pytest
import torch

from mi355.synth import randn, synth_state_dict
from tests.test_classcond_cpu import classcond_cfg, classcond_forward, load_case
from tests.test_gpu_classcond import _model, _report
from tests.test_rk_cpu import fixed_rk_ref, ref_tableau

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32 = dict(rtol=5e-4, atol=1e-4)
EPS32 = float(torch.finfo(torch.float32).eps)


@pytest.fixture(scope="module")
def ops():
    from mi355.ops import default_ops

    return default_ops


# ---- the stage op ---------------------------------------------------------------------------------------------------------------------

def _view(buf, n, aligned):
    """n elements of a guard-padded buffer: 16 bytes (fp32; 4 for uint8) into it, or one element in (4 bytes off the 16-byte grid)."""
    lo = 4 if aligned else 1
    return buf[lo:lo + n], lo


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("nk", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 5, 4099, 1 << 16])
def test_stage_op_vs_fp64(ops, n, nk, inplace):
    aligned = n != 4099     # 4099: every tensor a view 4 bytes off the 16-byte grid -> the scalar path (and n % 4 != 0)
    nan = float("nan")
    coeffs = [float(torch.tensor(c, dtype=torch.float32)) for c in (0.0625, -0.3, 1.7, 0.011)][:nk]
    src = [randn(6000 + s, n + 8).to(DEV) for s in range(nk + 1)]
    ks = [_view(b, n, aligned)[0] for b in src[:nk]]
    ybuf = torch.full((n + 8,), nan, device=DEV)
    y0, lo = _view(ybuf, n, aligned)
    y0.copy_(_view(src[nk], n, aligned)[0])
    y0_before = y0.clone()
    obuf, cbuf = torch.full((n + 8,), nan, device=DEV), torch.full((n + 8,), nan, device=DEV)
    ubuf = torch.full((n + 8,), 0x5A, dtype=torch.uint8, device=DEV)
    out = y0 if inplace else _view(obuf, n, aligned)[0]
    copy_out, u8_out = _view(cbuf, n, aligned)[0], _view(ubuf, n, aligned)[0]
    assert (out.data_ptr() % 16 == 0) == aligned and all((k.data_ptr() % 16 == 0) == aligned for k in ks)
    ops.rk_stage(out, y0, ks, coeffs, copy_out=copy_out, u8_out=u8_out)
    want = y0_before.double()
    mag = y0_before.double().abs()
    for k, c in zip(ks, coeffs):
        want = want + k.double() * c
        mag = mag + (k.double() * c).abs()
    err = (out.double() - want).abs()
    bound = (nk + 1) * EPS32 * mag
    print(f"rk_stage n={n} nk={nk} inplace={inplace}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(copy_out, out)
    assert torch.equal(u8_out, ops.quantize_u8(out.contiguous().clone()))
    for buf in (cbuf, ybuf) + (() if inplace else (obuf,)):      # guards on both sides of every output stay NaN
        assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + n:]).all())
    if inplace:
        assert bool(torch.isnan(obuf).all())
    assert bool((ubuf[:lo] == 0x5A).all()) and bool((ubuf[lo + n:] == 0x5A).all())
    # without the fused outputs: the same state, nothing else written
    again = torch.full((n + 8,), nan, device=DEV)
    o2 = _view(again, n, aligned)[0]
    y2 = y0_before.clone() if aligned else y0_before
    ops.rk_stage(o2, y2, ks, coeffs)
    assert torch.equal(o2, out)


def test_stage_op_arguments(ops):
    from mi355 import _lib

    L = _lib.lib()
    x = torch.zeros(8, device=DEV)
    with pytest.raises(ValueError):
        ops.rk_stage(x, x, [], [])
    with pytest.raises(ValueError):
        ops.rk_stage(x, x, [x] * 5, [1.0] * 5)
    kp = (C.c_void_p * 4)(x.data_ptr(), None, None, None)
    cf = (C.c_float * 4)(1.0, 0.0, 0.0, 0.0)
    p = C.c_void_p(x.data_ptr())
    assert L.mi355_rk_stage(p, p, kp, cf, 0, 8, None, None, None) < 0 and b"rk_stage" in L.mi355_last_error()
    assert L.mi355_rk_stage(p, p, kp, cf, 2, 8, None, None, None) < 0 and b"null" in L.mi355_last_error()
    assert L.mi355_rk_stage(None, p, kp, cf, 1, 8, None, None, None) < 0
    assert L.mi355_rk_stage(None, None, kp, cf, 1, 0, None, None, None) == 0      # n <= 0: nothing to do
    ops.rk_stage(x, x, [torch.ones(8, device=DEV)], [2.0])
    assert torch.equal(x, torch.full((8,), 2.0, device=DEV))


# ---- the whole sampler ----------------------------------------------------------------------------------------------------------------

GRIDS = [[0.0, 1.0], [0.0, 0.05, 0.07, 0.5, 1.0]]
_CACHE = {}


def _net(golden, kind, precision="fp32"):
    """kind: "mnist" (unet_mnist's config), "mnist_cc" (its class-conditional case), "cond" (tiny, 1 state + 1 condition channel), "cond_x2"
    (the same with out.2 doubled: over the uneven grid the plain field is too flat for _assert_teeth, midpoint and rk4 being 6.1 x the
    tolerance apart; doubled they are 37 x apart).  -> (cfg, model, sd, B, labels, cond), built once per module."""
    key = (kind, precision)
    if key not in _CACHE:
        if kind == "mnist_cc":
            cfg = load_case(golden, "mnist")[1]
        else:
            cfg = classcond_cfg(golden("unet_mnist" if kind == "mnist" else "unet_tiny_in2").json("config"))
        seed = {"mnist": 5101, "mnist_cc": 5102, "cond": 5103, "cond_x2": 5103}[kind]
        sd = None
        if kind == "cond_x2":
            from image_diffusion.unet import param_shapes

            sd = dict(synth_state_dict(param_shapes(cfg), seed))
            sd["out.2.weight"], sd["out.2.bias"] = sd["out.2.weight"] * 2.0, sd["out.2.bias"] * 2.0
        m, sd = _model(cfg, seed, precision, sd)
        B = 3 if kind.startswith("cond") else 4
        y = torch.tensor([3, 0, 9, 3]) if kind == "mnist_cc" else None
        cond = randn(5201, B, cfg.in_channels - cfg.out_channels, cfg.image_size, cfg.image_size) if kind.startswith("cond") else None
        _CACHE[key] = (cfg, m, sd, B, y, cond)
    return _CACHE[key]


def _x0(cfg, B, seed=5200):
    return randn(seed, B, cfg.out_channels, cfg.image_size, cfg.image_size)


def _ref(golden, kind, grid, method, B=None, y=None, seed=5200):
    """fixed_rk_ref over the oracle's U-Net (fp32, CPU), every state; computed once and shared (never modified)."""
    key = ("ref", kind, tuple(grid), method, B, seed)
    if key not in _CACHE:
        cfg, _, sd, B0, y0, cond = _net(golden, kind)
        B = B or B0
        y = y0 if y is None else y
        x0 = _x0(cfg, B, seed)
        f = lambda t, x: classcond_forward(sd, cfg, x if cond is None else torch.cat((x, cond), dim=1), t.reshape(1).repeat(B), y)  # noqa: E731
        _CACHE[key] = fixed_rk_ref(f, x0, grid, ref_tableau(method))
    return _CACHE[key]


def _assert_teeth(golden, kind, grid):
    """The comparison can tell the methods apart: on these inputs the restatements of euler, midpoint and rk4 differ pairwise by at least
    10x the tolerance (max abs; the tolerance at the largest reference value)."""
    refs = {m: _ref(golden, kind, grid, m)[-1] for m in ("euler", "midpoint", "rk4")}
    tol = FP32["atol"] + FP32["rtol"] * max(float(r.abs().max()) for r in refs.values())
    names = list(refs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            d = float((refs[a] - refs[b]).abs().max())
            print(f"{kind} {grid}: |{a} - {b}| = {d:.3e} = {d / tol:.1f} x tolerance")
            assert d >= 10 * tol, (kind, grid, a, b, d, tol)


SAMPLER_CASES = [(kind, g, m) for kind in ("mnist", "mnist_cc") for g in range(2) for m in ("midpoint", "rk4", "rk4_38")] + \
                [("cond", 0, m) for m in ("midpoint", "rk4", "rk4_38")] + \
                [("cond_x2", 1, m) for m in ("heun2", "rk4")]      # the condition across several uneven steps; heun2's second stage sits at t[k+1]


@pytest.mark.parametrize("kind,g,method", SAMPLER_CASES)
def test_sampler_fp32_vs_restatement(golden, ops, kind, g, method):
    """UNetEngine.cfm_rk (one library call) against the restatement: the final state and every trajectory entry; traj[0] the input and
    traj[-1] the state exactly; the uint8 output the quantised state.  (mnist, second grid, rk4) also runs in slices."""
    grid = GRIDS[g]
    cfg, m, sd, B, y, cond = _net(golden, kind)
    _assert_teeth(golden, kind, grid)
    ref = _ref(golden, kind, grid, method)
    eng = m.engine(DEV)
    x0 = _x0(cfg, B)
    kw = dict(cond=cond.to(DEV) if cond is not None else None, y=y.to(DEV) if y is not None else None)
    x = x0.to(DEV)
    xr, traj, u8 = eng.cfm_rk(x, grid, method, keep_traj=True, want_u8=True, **kw)
    assert xr is x
    _report(f"cfm_rk {kind} grid {g} {method} final", x.cpu(), ref[-1])
    torch.testing.assert_close(x.cpu(), ref[-1], **FP32)
    assert traj.shape == (len(grid),) + tuple(x0.shape)
    assert torch.equal(traj[0].cpu(), x0) and torch.equal(traj[-1], x)
    for k in range(len(grid)):
        torch.testing.assert_close(traj[k].cpu(), ref[k], **FP32)
    assert u8.dtype == torch.uint8 and torch.equal(u8, ops.quantize_u8(x))
    x2 = x0.to(DEV)      # without the optional outputs: the same state
    _, t2, u2 = eng.cfm_rk(x2, grid, method, **kw)
    assert t2 is None and u2 is None and torch.equal(x2, x)
    if (kind, g, method) == ("mnist", 1, "rk4"):
        eng.max_batch_override = 3
        try:
            xs = x0.to(DEV)
            _, trs, us = eng.cfm_rk(xs, grid, method, keep_traj=True, want_u8=True)
        finally:
            eng.max_batch_override = None
        torch.testing.assert_close(xs.cpu(), ref[-1], **FP32)
        torch.testing.assert_close(trs.cpu(), traj.cpu(), rtol=1e-5, atol=1e-6)
        assert torch.equal(us, ops.quantize_u8(xs))
    torch.cuda.synchronize()
    eng.check()


def test_single_time_is_a_no_op(golden, ops):
    """n_t == 1: no step; traj[0] and the uint8 output are still written."""
    cfg, m, _, B, _, _ = _net(golden, "mnist")
    x0 = _x0(cfg, B).to(DEV)
    x = x0.clone()
    _, traj, u8 = m.engine(DEV).cfm_rk(x, [0.3], "rk4", keep_traj=True, want_u8=True)
    assert torch.equal(x, x0) and traj.shape[0] == 1 and torch.equal(traj[0], x0) and torch.equal(u8, ops.quantize_u8(x0))


def test_euler_through_the_tableau(golden):
    """cfm_rk(method="euler") against cfm_euler (which rounds inside the last conv's epilogue: no bit equality asked) and the restatement."""
    cfg, m, _, B, _, _ = _net(golden, "mnist")
    eng = m.engine(DEV)
    grid = GRIDS[1]
    xa, xb = _x0(cfg, B).to(DEV), _x0(cfg, B).to(DEV)
    _, ta, _ = eng.cfm_rk(xa, grid, "euler", keep_traj=True)
    _, tb, _ = eng.cfm_euler(xb, grid, keep_traj=True)
    _report("euler tableau vs cfm_euler", xa.cpu(), xb.cpu())
    torch.testing.assert_close(ta, tb, **FP32)
    torch.testing.assert_close(xa.cpu(), _ref(golden, "mnist", grid, "euler")[-1], **FP32)


def test_fast_path_vs_host_loop():
    """NeuralODE(wrapper, solver="rk4").trajectory is one library call; FixedStepRK over engine.forward is the host-driven loop (one
    forward and one rk_stage launch per stage)."""
    from mi355.ode import FixedStepRK
    from tests.test_gpu_sde import _wrappers
    from torchcfm_compat import NeuralODE

    (m,) = _wrappers(False, (5301,))
    x0 = randn(5302, 5, 1, 28, 28).to(DEV)
    ts = torch.tensor([0.0, 0.2, 0.25, 1.0])
    fast = NeuralODE(m, solver="rk4").trajectory(x0, ts)
    eng = m.engine(DEV)
    sol = FixedStepRK(lambda t, y: [eng.forward(y[0], float(t))], "rk4")
    host = torch.stack([x0] + [s[0] for s in sol.integrate_times([x0], ts.tolist())])
    assert sol.nfe == 12 and fast.shape == host.shape == (4, 5, 1, 28, 28)
    _report("rk4 fast path vs host loop", fast.cpu(), host.cpu())
    torch.testing.assert_close(fast, host, rtol=1e-4, atol=1e-4)
    assert torch.equal(fast[0], x0) and (fast[-1] - x0).abs().max() > 1e-2
    # a callable that is no wrapper takes the host loop inside NeuralODE: the same numbers again
    plain = NeuralODE(lambda t, x: m(t, x), solver="rk4").trajectory(x0, ts)
    torch.testing.assert_close(plain, host, rtol=1e-4, atol=1e-4)


def test_beyond_the_embedding_table(golden):
    """26 rk4 steps with labels: 26 * 4 * 10 = 1040 (step, stage, class) rows > 1024, so every evaluation computes its own embedding."""
    cfg, m, sd, _, _, _ = _net(golden, "mnist_cc")
    B = 2
    y = torch.tensor([7, 2])
    grid = torch.linspace(0, 1, 27).tolist()
    assert (len(grid) - 1) * 4 * cfg.num_classes > 1024
    ref = _ref(golden, "mnist_cc", grid, "rk4", B=B, y=y, seed=5400)
    x = _x0(cfg, B, 5400).to(DEV)
    eng = m.engine(DEV)
    eng.cfm_rk(x, grid, "rk4", y=y.to(DEV))
    _report("rk4 26 steps, labels, per-evaluation embedding", x.cpu(), ref[-1])
    torch.testing.assert_close(x.cpu(), ref[-1], **FP32)
    torch.cuda.synchronize()
    eng.check()


def test_sampler_bf16_vs_restatement(golden):
    cfg, m, _, B, _, _ = _net(golden, "mnist", "bf16")
    grid = torch.linspace(0, 1, 4).tolist()
    _net(golden, "mnist")      # the restatement reads the fp32 case's state dict: the same seed, the same weights
    ref = _ref(golden, "mnist", grid, "rk4")
    x = _x0(cfg, B).to(DEV)
    m.engine(DEV).cfm_rk(x, grid, "rk4")
    emax, scale, rms = _report("cfm_rk bf16 3-step rk4", x.cpu(), ref[-1])
    assert emax < 0.03 * scale and rms < 0.01


def test_make_gen_1_img_midpoint():
    """compute_fid's --integration_method midpoint at the shape of the Euler test of test_gpu_configs.py: uint8 [B, 3, 32, 32],
    deterministic under a seed, the next call a fresh batch, and not Euler's images."""
    import compute_fid
    from image_diffusion.unet import param_shapes

    net = compute_fid.build_model(128, DEV, precision="fp32")
    net.load_state_dict(synth_state_dict(param_shapes(net), 1234))
    B, steps = 40, 8
    gen = compute_fid.make_gen_1_img(net, batch_size_fid=B, integration_steps=steps, integration_method="midpoint", device=DEV, seed=11)
    img = gen(None)
    assert img.dtype == torch.uint8 and img.shape == (B, 3, 32, 32) and img.device.type == "cuda"
    again = compute_fid.make_gen_1_img(net, batch_size_fid=B, integration_steps=steps, integration_method="midpoint", device=DEV, seed=11)(None)
    assert torch.equal(img, again)
    assert not torch.equal(gen(None), img)
    euler = compute_fid.make_gen_1_img(net, batch_size_fid=B, integration_steps=steps, integration_method="euler", device=DEV, seed=11)(None)
    assert not torch.equal(euler, img)
    x = compute_fid.draw_x0_shard(B, 11, 0, torch.device(DEV))
    _, _, want = net.engine(DEV).cfm_rk(x, torch.linspace(0, 1, steps + 1).tolist(), "midpoint", want_u8=True)
    assert torch.equal(img, want)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals(golden):
    """Argument errors of mi355_cfm_rk_sample: an error code and a text each, nothing launched; the handle stays usable."""
    cfg, m, _, B, _, _ = _net(golden, "mnist")
    eng = m.engine(DEV)
    L = eng.L
    x0 = _x0(cfg, B).to(DEV)
    x = x0.clone()
    a, b, c = ref_tableau("rk4")
    fa = (C.c_float * 25)(*([v for r in a for v in r] + [0.0] * 9))
    fb, fc = (C.c_float * 5)(*(b + [0.0])), (C.c_float * 5)(*(c + [0.0]))
    ts = (C.c_float * 2)(0.0, 1.0)
    ws, wsb = eng._workspace_rk(B, 4)
    need = L.mi355_cfm_rk_workspace_bytes(eng.handle, B, 4)
    base = L.mi355_unet_workspace_bytes(eng.handle, B)
    state = B * 28 * 28 * 4
    assert need == (base + 255) // 256 * 256 + 5 * ((state + 255) // 256 * 256)
    lab = torch.zeros(B, dtype=torch.int32, device=DEV)
    xp = C.c_void_p(x.data_ptr())

    def call(stages=4, labels=None, xc=1, bytes_=wsb, pa=fa):
        return L.mi355_cfm_rk_sample(eng.handle, xp, xc, None, 0, labels, ts, 2, stages, pa, fb, fc, None, None, B, ws, bytes_, eng._stream())

    for kwargs, text in ((dict(stages=0), b"1 to 4 stages"), (dict(stages=5), b"1 to 4 stages"), (dict(pa=None), b"null tableau"),
                         (dict(bytes_=need - 1), b"workspace too small"), (dict(labels=C.c_void_p(lab.data_ptr())), b"num_classes"),
                         (dict(xc=2), b"channel count")):
        rc = call(**kwargs)
        assert rc < 0 and text in L.mi355_last_error(), (kwargs, rc, L.mi355_last_error())
    assert L.mi355_cfm_rk_workspace_bytes(eng.handle, B, 0) < 0 and L.mi355_cfm_rk_workspace_bytes(eng.handle, B, 5) < 0
    torch.cuda.synchronize()
    assert torch.equal(x, x0)      # nothing ran
    eng.check()
    assert call() == 0             # the handle is still usable: a valid call, and the same numbers as through the engine
    torch.cuda.synchronize()
    eng.check()
    torch.testing.assert_close(x.cpu(), _ref(golden, "mnist", [0.0, 1.0], "rk4")[-1], **FP32)
    fb0 = (C.c_float * 5)()        # weights that are all zero: refused, not run as x + 0 * k_1
    rc = L.mi355_cfm_rk_sample(eng.handle, xp, 1, None, 0, None, ts, 2, 4, fa, fb0, fc, None, None, B, ws, wsb, eng._stream())
    assert rc < 0 and b"all zero" in L.mi355_last_error()
    assert call() == 0
    torch.cuda.synchronize()
    eng.check()
    with pytest.raises(NotImplementedError):
        eng.cfm_rk(x, [0.0, 1.0], "rk5")
    with pytest.raises(ValueError, match="num_classes"):
        eng.cfm_rk(x, [0.0, 1.0], "rk4", y=lab)
