"""GPU: the SF2M stochastic sampler of the torchcfm notebooks (torchsde.sdeint of drift = model + score_model, g = sigma) on the HIP path.

- the Euler-Maruyama step op (mi355_sde_euler_step) bit for bit against the eager torch expression torchsde's Euler step evaluates, and
  its Philox noise (determinism, moments, independence of successive step offsets);
- the two-network loop (mi355_sf2m_euler_sample) with injected increments against tests.test_sde_cpu.sf2m_euler_ref, the fp32 restatement
  over the oracle's U-Net: unconditional and with labels, reverse, interpolated output times, bf16;
- torchsde_compat.sdeint's one-call fast path against its host-driven loop over the notebook's own SDE class, the notebook's cell at its
  size, the noise scale with a zero drift, and the library's refusals.

Tolerances: fp32 the CFM Euler bound of test_gpu_configs.py (rtol 5e-4, atol 1e-4); bf16 its 3-step Euler bounds (max 3 % of scale,
rms 1 %).
"""
import math

import pytest
import torch

from mi355.synth import rand_uniform, randn, synth_state_dict
from tests.test_classcond_cpu import ClassCondConfig, classcond_cfg, load_case
from tests.test_gpu_classcond import _model, _report
from tests.test_sde_cpu import sf2m_euler_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32 = dict(rtol=5e-4, atol=1e-4)


@pytest.fixture(scope="module")
def ops():
    from mi355.ops import default_ops

    return default_ops


def _neg(v, c):
    return -v if c < 0 else v


# ---- the step op ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g_tensor", [False, True])
@pytest.mark.parametrize("signs", [(1.0, None), (-1.0, None), (1.0, 1.0), (-1.0, 1.0), (1.0, -1.0)])
@pytest.mark.parametrize("n", [1 << 16, 78400 + 3, 5])
def test_step_op_bit_exact_vs_eager(ops, n, signs, g_tensor):
    """x + f * dt + g * dW with f = (+-a) (+ (+-b)) summed first, as torchsde's Euler step over the notebook's f: bit-exact."""
    ca, cb = signs
    x, a, b, dW = (randn(100 + s, n).to(DEV) for s in range(4))
    dW = dW * 0.1
    g = rand_uniform(104, 0.05, 0.3, n).to(DEV) if g_tensor else 0.1
    dt = torch.tensor(0.01, dtype=torch.float32, device=DEV)   # a step length as torchsde holds it (t1 - t0, fp32)
    f = _neg(a, ca) if cb is None else _neg(a, ca) + _neg(b, cb)
    want = x + f * dt + g * dW
    got = x.clone()
    ops.sde_euler_step_(got, a, float(dt), g, b=b if cb is not None else None, ca=ca, cb=cb or 1.0, dW=dW)
    assert torch.equal(got, want)


def test_step_op_unaligned_views_and_output_times(ops):
    """Views 4 bytes off the 16-byte grid and n % 4 != 0; the output write x_k + w (x_{k+1} - x_k) of the same launch (w = 0 / 1: the end
    points exactly); the guard elements around every output stay untouched."""
    n = 4099
    x0, a, b, dW = (randn(200 + s, n + 1).to(DEV)[1:] for s in range(4))
    dt = 0.03125
    want1 = x0 + (a + b) * dt + 0.1 * dW
    for w in (0.0, 0.375, 0.3, 1.0):
        xb = torch.empty(n + 2, device=DEV)
        xb[1:-1] = x0
        xs = xb[1:-1]
        ob = torch.full((n + 2,), float("nan"), device=DEV)
        out = ob[1:-1]
        ops.sde_euler_step_(xs, a, dt, 0.1, b=b, dW=dW, out=out, w=w)
        assert torch.equal(xs, want1)
        wantw = x0 if w == 0.0 else (want1 if w == 1.0 else x0 + torch.tensor(w, device=DEV) * (want1 - x0))
        assert torch.equal(out, wantw), w
        assert torch.isnan(ob[0]) and torch.isnan(ob[-1])


def test_step_op_philox(ops):
    """Device noise: dW = sqrt(dt) z with z the mi355_randn stream at (seed, offset) - bit-exact against the eager expression over that
    stream; the same seed reproduces, another differs; over 2^20 draws the mean and variance of dW / sqrt(dt) are within 5 sigma of 0 and
    1 and successive step offsets (k * n) are uncorrelated."""
    n = 1 << 20
    zero = torch.zeros(n, device=DEV)

    def draw(seed, off):
        x = zero.clone()
        ops.sde_euler_step_(x, zero, 0.25, 1.0, philox=(seed, off))   # 0 + 0 * dt + 1 * (0.5 z): exactly z / 2
        return x * 2.0

    z1, z2, z3, z4 = draw(7, 0), draw(7, 0), draw(8, 0), draw(7, n)
    assert torch.equal(z1, z2)
    assert float((z1 != z3).float().mean()) > 0.99
    assert torch.equal(z4, ops.randn((n,), DEV, seed=7, offset=n))
    N = float(n)
    for z in (z1, z4):
        m, v = float(z.double().mean()), float(z.double().var())
        print(f"philox dW/sqrt(dt): mean {m:.2e} var {v:.5f}")
        assert abs(m) < 5 / math.sqrt(N) and abs(v - 1.0) < 5 * math.sqrt(2 / N)
    corr = float((z1.double() * z4.double()).mean())
    assert abs(corr) < 5 / math.sqrt(N), corr
    # a general step over the same stream, against the eager expression (sqrt(dt) rounded on the host, as the launch does)
    x, a, b = (randn(300 + s, n).to(DEV) for s in range(3))
    dt = 0.01
    sdt = float(torch.tensor(dt, dtype=torch.float32).sqrt())
    r = ops.randn((n,), DEV, seed=11, offset=3 * n)
    want = x + (-a + b) * torch.tensor(dt, device=DEV) + 0.1 * (sdt * r)
    got = x.clone()
    ops.sde_euler_step_(got, a, dt, 0.1, b=b, ca=-1.0, philox=(11, 3 * n))
    assert torch.equal(got, want)


# ---- the whole sampler ----------------------------------------------------------------------------------------------------------------

def _nets(golden, conditional, precision):
    if conditional:
        _, cfg = load_case(golden, "mnist")
    else:
        cfg = classcond_cfg(golden("unet_mnist").json("config"))
    d, dsd = _model(cfg, 4101, precision)
    s, ssd = _model(cfg, 4102, precision)
    return cfg, d, dsd, s, ssd


CASES = [   # conditional, reverse, ts, dt
    (False, False, [0.0, 1.0], 0.1),
    (True, False, [0.0, 1.0], 0.1),
    (False, True, [0.0, 1.0], 0.1),
    (True, True, [0.0, 0.05, 0.07, 0.5, 1.0], 0.1),
    (False, False, [0.0, 0.05, 0.07, 0.5, 1.0], 0.1),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_sampler_fp32_vs_restatement(golden, case):
    """UNetEngine.sf2m_euler (one library call) with injected increments against the fp32 restatement: final state and every output time
    (several inside the first step: the interpolation of the fused launch and of its re-run on a copy).  Case 0 also runs in slices."""
    from torchsde_compat import step_grid

    conditional, reverse, ts, dt = CASES[case]
    cfg, d, dsd, s, ssd = _nets(golden, conditional, "fp32")
    B = 4
    grid, outs = step_grid(ts, dt)
    n = len(grid) - 1
    x0 = randn(4200 + case, B, 1, 28, 28)
    dW = randn(4300 + case, n, B, 1, 28, 28) * math.sqrt(dt)
    y = torch.tensor([3, 0, 9, 3]) if conditional else None
    ref, refo = sf2m_euler_ref(dsd, ssd, cfg, x0, grid, dW, 0.1, reverse, y, outs)
    ed, es = d.engine(DEV), s.engine(DEV)
    x = x0.to(DEV)
    _, traj = ed.sf2m_euler(es, x, grid, 0.1, reverse, y=y.to(DEV) if y is not None else None, dW=dW.to(DEV), outputs=outs)
    _report(f"sf2m case {case} fp32 final", x.cpu(), ref)
    torch.testing.assert_close(x.cpu(), ref, **FP32)
    assert traj.shape == (len(outs), B, 1, 28, 28)
    assert torch.equal(traj[0].cpu(), x0) and torch.equal(traj[-1], x)
    for j in range(len(outs)):
        torch.testing.assert_close(traj[j].cpu(), refo[j], **FP32)
    if case == 0:
        ed.max_batch_override = 3
        try:
            xs = x0.to(DEV)
            _, trs = ed.sf2m_euler(es, xs, grid, 0.1, reverse, dW=dW.to(DEV), outputs=outs)
        finally:
            ed.max_batch_override = None
        torch.testing.assert_close(xs.cpu(), ref, **FP32)
        torch.testing.assert_close(trs.cpu(), traj.cpu(), rtol=1e-5, atol=1e-6)
    torch.cuda.synchronize()
    ed.check()
    es.check()


@pytest.mark.parametrize("conditional", [False, True])
def test_sampler_bf16_vs_restatement(golden, conditional):
    from torchsde_compat import step_grid

    cfg, d, dsd, s, ssd = _nets(golden, conditional, "bf16")
    B = 4
    grid, _ = step_grid([0.0, 1.0], 0.1)
    n = len(grid) - 1
    x0 = randn(4401, B, 1, 28, 28)
    dW = randn(4402, n, B, 1, 28, 28) * math.sqrt(0.1)
    y = torch.tensor([1, 5, 5, 8]) if conditional else None
    ref, _ = sf2m_euler_ref(dsd, ssd, cfg, x0, grid, dW, 0.1, False, y)
    x = x0.to(DEV)
    d.engine(DEV).sf2m_euler(s.engine(DEV), x, grid, 0.1, y=y.to(DEV) if y is not None else None, dW=dW.to(DEV))
    emax, scale, rms = _report(f"sf2m bf16 conditional={conditional}", x.cpu(), ref)
    assert emax < 0.03 * scale and rms < 0.01


# ---- the torchsde front end -----------------------------------------------------------------------------------------------------------

class NotebookSDE(torch.nn.Module):
    """conditional_mnist.ipynb's SDE class as written there (mnist_example.ipynb's is the same without labels)."""

    noise_type = "diagonal"
    sde_type = "ito"

    def __init__(self, ode_drift, score, labels=None, reverse=False, sigma=0.1):
        super().__init__()
        self.drift = ode_drift
        self.score = score
        self.reverse = reverse
        self.labels = labels
        self.sigma = sigma

    def f(self, t, y):
        y = y.view(-1, 1, 28, 28)
        if self.reverse:
            t = 1 - t
            return -self.drift(t, y, self.labels) + self.score(t, y, self.labels)
        return self.drift(t, y, self.labels).flatten(start_dim=1) + self.score(t, y, self.labels).flatten(start_dim=1)

    def g(self, t, y):
        return torch.ones_like(y) * self.sigma


class GridBM:
    """torchsde's Brownian interface bm(ta, tb) -> W(tb) - W(ta), for the step boundaries of one grid: increments drawn once."""

    def __init__(self, grid, shape, seed):
        self.t = [float(v) for v in grid]
        self.inc = [randn(seed + k, *shape) * math.sqrt(self.t[k + 1] - self.t[k]) for k in range(len(grid) - 1)]

    def __call__(self, ta, tb):
        k = self.t.index(float(ta))
        assert float(tb) == self.t[k + 1]
        return self.inc[k].to(DEV)


def _wrappers(conditional, seeds, precision="fp32", zero_out=False):
    from image_diffusion.unet import param_shapes
    from torchcfm_compat import ClassCondUNetModelWrapper, UNetModelWrapper

    kw = dict(dim=(1, 28, 28), num_channels=32, num_res_blocks=1, precision=precision)
    cls = ClassCondUNetModelWrapper if conditional else UNetModelWrapper
    if conditional:
        kw.update(num_classes=10, class_cond=True)
    nets = []
    for sd_seed in seeds:
        m = cls(**kw)
        sd = synth_state_dict(param_shapes(m), sd_seed)
        if zero_out:
            sd["out.2.weight"].zero_()
            sd["out.2.bias"].zero_()
        m.load_state_dict(sd)
        nets.append(m.to(DEV))
    return nets


@pytest.mark.parametrize("conditional", [False, True])
def test_fast_path_vs_host_driven_notebook_class(conditional):
    """sdeint(SF2MSDE(model, score_model)) is one library call; sdeint over the notebook's own SDE class is the host-driven loop
    (f, g, step op).  Same bm: the same increments; bm=None: the same torch seed gives both the same device stream.  Reverse: SF2MSDE over
    plain callables (host-driven) against SF2MSDE over the wrappers (one call)."""
    from torchsde_compat import SF2MSDE, sdeint, step_grid

    m, sm = _wrappers(conditional, (4501, 4502))
    B = 10
    labels = torch.arange(10, device=DEV) if conditional else None
    y0 = randn(4503, B, 784).to(DEV)
    ts = torch.linspace(0, 1, 3, device=DEV)
    dt = 0.05
    grid, outs = step_grid(ts, dt)
    assert 0 < outs[1][1] < 1   # the middle output time falls inside a step
    bm = GridBM(grid, (B, 784), 4504)
    fast = sdeint(SF2MSDE(m, sm, labels=labels, sigma=0.1), y0, ts, bm=bm, dt=dt)
    host = sdeint(NotebookSDE(m, sm, labels=labels, sigma=0.1), y0, ts, bm=bm, dt=dt)
    assert fast.shape == host.shape == (3, B, 784)
    _report(f"fast vs host-driven (conditional={conditional})", fast.cpu(), host.cpu())
    torch.testing.assert_close(fast, host, rtol=1e-4, atol=1e-4)
    assert torch.equal(fast[0], y0)
    torch.manual_seed(5)
    a = sdeint(SF2MSDE(m, sm, labels=labels, sigma=0.1), y0, ts, dt=dt)
    torch.manual_seed(5)
    b = sdeint(NotebookSDE(m, sm, labels=labels, sigma=0.1), y0, ts, dt=dt)
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)
    torch.manual_seed(6)
    c = sdeint(SF2MSDE(m, sm, labels=labels, sigma=0.1), y0, ts, dt=dt)
    assert (c - a).abs().max() > 1e-2
    rev_fast = sdeint(SF2MSDE(m, sm, labels=labels, reverse=True, sigma=0.1), y0, ts, bm=bm, dt=dt)
    rev_host = sdeint(SF2MSDE(lambda t, x, y=None: m(t, x, y), lambda t, x, y=None: sm(t, x, y), labels=labels, reverse=True, sigma=0.1),
                      y0, ts, bm=bm, dt=dt)
    torch.testing.assert_close(rev_fast, rev_host, rtol=1e-4, atol=1e-4)
    assert (rev_fast - fast).abs().max() > 1e-2


def test_notebook_cell_runs():
    """conditional_mnist.ipynb's SDE cell after `from torchsde_compat import sdeint, SF2MSDE as SDE`: B = 100, labels arange(10).repeat(10),
    ts = linspace(0, 1, 2), dt = 0.01 (101 steps), the wrappers' default precision."""
    from torchsde_compat import SF2MSDE as SDE
    from torchsde_compat import sdeint

    model, score_model = _wrappers(True, (4601, 4602), precision=None)
    sde = SDE(model, score_model, labels=torch.arange(10, device=DEV).repeat(10), sigma=0.1)
    y0 = torch.randn(100, 1 * 28 * 28, device=DEV)
    with torch.no_grad():
        sde_traj = sdeint(sde, y0, ts=torch.linspace(0, 1, 2, device=DEV), dt=0.01)
    assert sde_traj.shape == (2, 100, 784)
    assert torch.equal(sde_traj[0], y0) and bool(torch.isfinite(sde_traj).all())
    model.engine(DEV).check()


def test_zero_drift_gives_sigma_squared_variance():
    """out.2 of both nets zeroed: the drift is 0, so x_1 - x_0 = sigma * sum_k dW_k with sum dt_k = 1: per-element variance sigma^2
    within 3 % (78 400 elements; 6 sigma of the estimate), device Philox noise, 101 steps."""
    from torchsde_compat import SF2MSDE, sdeint

    m, sm = _wrappers(False, (4701, 4702), zero_out=True)
    y0 = randn(4703, 100, 784).to(DEV)
    torch.manual_seed(4704)
    traj = sdeint(SF2MSDE(m, sm, sigma=0.1), y0, torch.linspace(0, 1, 2), dt=0.01)
    dx = (traj[-1] - y0).double()
    var, mean = float(dx.var()), float(dx.mean())
    print(f"zero drift: var {var:.6f} (sigma^2 = 0.01), mean {mean:.2e}")
    assert abs(var / 0.01 - 1.0) < 0.03 and abs(mean) < 5 * 0.1 / math.sqrt(dx.numel())


def test_refusals(golden):
    """Mismatched nets, labels with only one class-conditional net, and a label out of range: MI355BackendError naming the cause."""
    from mi355._lib import MI355BackendError

    _, cfg_c = load_case(golden, "mnist")
    cfg_u = classcond_cfg(golden("unet_mnist").json("config"))
    cond, _ = _model(cfg_c, 4801, "fp32")
    cond2, _ = _model(cfg_c, 4802, "fp32")
    unc, _ = _model(cfg_u, 4803, "fp32")
    small, _ = _model(ClassCondConfig(16, 1, 32, 1, 1, (2,), channel_mult=(1, 2)), 4804, "fp32")
    x = randn(4805, 2, 1, 28, 28).to(DEV)
    grid = [0.0, 0.5, 1.0]
    y = torch.tensor([1, 2], device=DEV)
    with pytest.raises(MI355BackendError, match="differ"):
        unc.engine(DEV).sf2m_euler(small.engine(DEV), x.clone(), grid, 0.1, seed=1)
    with pytest.raises(MI355BackendError, match="num_classes"):
        cond.engine(DEV).sf2m_euler(unc.engine(DEV), x.clone(), grid, 0.1, y=y, seed=1)
    with pytest.raises(MI355BackendError, match="num_classes"):
        unc.engine(DEV).sf2m_euler(cond.engine(DEV), x.clone(), grid, 0.1, y=y, seed=1)
    e1, e2 = cond.engine(DEV), cond2.engine(DEV)
    with pytest.raises(MI355BackendError, match="label"):
        e1.sf2m_euler(e2, x.clone(), grid, 0.1, y=torch.tensor([1, 10], device=DEV), seed=1)
        torch.cuda.synchronize()
        e1.check()
    torch.cuda.synchronize()
    for e in (e1, e2):   # both handles saw the label; a flag the sampler already reported may still be set
        try:
            e.check()
        except MI355BackendError:
            pass
        e.check()
