"""CPU: the SF2M stochastic sampler's host parts - torchsde's fixed-step grid as torchsde_compat restates it, sdeint's refusals, the
notebooks' SDE module (torchsde_compat.SF2MSDE), the new library symbols, and `sf2m_euler_ref`, the fp32 restatement of the whole sampler
that tests/test_gpu_sde.py holds the HIP loop to.

torchsde is not vendored: the grid rule (next_t = min(curr_t + dt, ts[-1]) on fp32 tensors, linear interpolation of output times inside a
step) and the Euler step y1 = y0 + f*dt + g*dW are restated from its fixed-step loop ('parity unpinned' against its default SRK solver).
"""
import math

import numpy as np
import pytest
import torch

from tests.test_classcond_cpu import classcond_forward


def sf2m_euler_ref(drift_sd, score_sd, cfg, x0, grid, dW, sigma, reverse=False, labels=None, outputs=(), forward=classcond_forward):
    """Euler-Maruyama of dx = (model(t, x) + score_model(t, x)) dt + sigma dW over the fp32 step boundaries `grid`, as the notebooks'
    torchsde.sdeint(SDE(model, score_model, labels, reverse, sigma), ...) evaluates it in eager fp32: f = drift + score (reverse: both nets
    at 1 - t, f = -drift + score), x_{k+1} = x_k + f * dt_k + sigma * dW[k].  outputs: (step k, weight w) pairs -> x_k + w * (x_{k+1} - x_k)
    (the end points themselves for w = 0 / 1).  forward(sd, cfg, x, t[B], labels) is the net (default: the oracle's U-Net with the label
    term).  -> (final state, [outputs])"""
    x = x0.float().clone()
    B = x.shape[0]
    outs = [None] * len(outputs)
    for k in range(len(grid) - 1):
        t0 = torch.tensor(grid[k], dtype=torch.float32)
        dt = torch.tensor(grid[k + 1], dtype=torch.float32) - t0
        te = (1 - t0) if reverse else t0
        tb = te.reshape(1).repeat(B)
        a = forward(drift_sd, cfg, x, tb, labels)
        b = forward(score_sd, cfg, x, tb, labels)
        f = -a + b if reverse else a + b
        x1 = x + f * dt + sigma * dW[k]
        for j, (kk, w) in enumerate(outputs):
            if kk == k:
                outs[j] = x.clone() if w == 0.0 else (x1.clone() if w == 1.0 else x + torch.tensor(w, dtype=torch.float32) * (x1 - x))
        x = x1
    return x, outs


# ---- the step grid ------------------------------------------------------------------------------------------------------------------

def test_grid_of_the_notebook_call():
    """ts = linspace(0, 1, 2), dt = 0.01: fp32 accumulation of curr_t gives 101 steps, the last 6.5565e-7 long."""
    from torchsde_compat import step_grid

    grid, outs = step_grid(torch.linspace(0, 1, 2), 0.01)
    assert len(grid) == 102
    last = float(np.float32(grid[-1]) - np.float32(grid[-2]))
    assert abs(last - 6.5565e-7) < 1e-10, last
    assert grid[-1] == 1.0 and grid[0] == 0.0
    assert outs == [(0, 0.0), (100, 1.0)]
    # every boundary is the fp32 sum of the one before and dt
    for k in range(100):
        assert np.float32(grid[k + 1]) == np.float32(np.float32(grid[k]) + np.float32(0.01))


def test_grid_with_several_output_times():
    """Output times inside a step are interpolated between the states around them; steps are not cut at output times (only at ts[-1])."""
    from torchsde_compat import step_grid

    grid, outs = step_grid([0.0, 0.005, 0.007, 0.5, 1.0], 0.01)
    assert len(grid) - 1 == 101
    assert [k for k, _ in outs] == [0, 0, 0, 50, 100]
    assert outs[0][1] == 0.0 and outs[-1][1] == 1.0
    w1 = float((torch.tensor(0.005) - torch.tensor(0.0)) / (torch.tensor(grid[1]) - torch.tensor(0.0)))
    assert outs[1][1] == w1 and abs(outs[2][1] - 0.7) < 1e-6
    assert grid[50] < 0.5 < grid[51] and 0 < outs[3][1] < 1e-3   # fp32 accumulation leaves t_50 just below 0.5
    # an output time that is a grid point: the state itself (weight 1 of the step that ends there)
    grid2, outs2 = step_grid([0.0, 0.25, 1.0], 0.125)
    assert grid2 == [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0]
    assert outs2 == [(0, 0.0), (1, 1.0), (7, 1.0)]


def test_grid_dt_larger_than_the_span():
    from torchsde_compat import step_grid

    grid, outs = step_grid([0.2, 0.7], 5.0)
    assert grid == [float(np.float32(0.2)), float(np.float32(0.7))]
    assert outs == [(0, 0.0), (0, 1.0)]
    grid, outs = step_grid([0.0, 0.3, 1.0], 2.0)   # one step; the inner output interpolated inside it
    assert len(grid) == 2 and [k for k, _ in outs] == [0, 0, 0] and abs(outs[1][1] - 0.3) < 1e-7


def test_grid_rejects_bad_times():
    from torchsde_compat import step_grid

    for ts in ([0.0], [0.0, 0.0], [1.0, 0.5]):
        with pytest.raises(ValueError):
            step_grid(ts, 0.1)
    with pytest.raises(ValueError):
        step_grid([0.0, 1.0], 0.0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

class _LinearSDE(torch.nn.Module):
    noise_type = "diagonal"
    sde_type = "ito"

    def f(self, t, y):
        return -y

    def g(self, t, y):
        return torch.ones_like(y) * 0.1


def test_sdeint_refusals():
    from mi355._lib import MI355BackendError
    from torchsde_compat import sdeint

    sde = _LinearSDE()
    y0 = torch.zeros(2, 4)
    ts = torch.linspace(0, 1, 2)
    for kw in (dict(method="srk"), dict(method="milstein"), dict(method="reversible_heun"), dict(adaptive=True), dict(logqp=True),
               dict(extra=True)):
        with pytest.raises(NotImplementedError):
            sdeint(sde, y0, ts, dt=0.01, **kw)
    for attr, val in (("sde_type", "stratonovich"), ("noise_type", "general"), ("noise_type", "scalar")):
        bad = _LinearSDE()
        setattr(bad, attr, val)
        with pytest.raises(NotImplementedError, match=attr):
            sdeint(bad, y0, ts, dt=0.01)
    with pytest.raises(MI355BackendError):       # no CPU path
        sdeint(sde, y0, ts, dt=0.01)
    with pytest.raises(MI355BackendError):
        sdeint(sde, y0, ts, method="euler", dt=0.01)


def test_step_op_refuses_cpu_tensors():
    from mi355._lib import MI355BackendError
    from mi355.ops import default_ops

    x = torch.zeros(8)
    with pytest.raises(MI355BackendError):
        default_ops.sde_euler_step_(x, torch.zeros(8), 0.1, 0.1, dW=torch.zeros(8))


# ---- the notebooks' SDE module ------------------------------------------------------------------------------------------------------

def test_sf2m_sde_module_drift_and_diffusion():
    """f = model + score on the image view of a flattened state, returned in the state's shape; reverse: both at 1 - t, -model + score;
    labels are passed to both models; g = sigma."""
    from torchsde_compat import SF2MSDE

    seen = []

    def model(t, x, y=None):
        seen.append(("m", tuple(x.shape), float(t), None if y is None else y.tolist()))
        return 2.0 * x + t

    def score(t, x, y=None):
        seen.append(("s", tuple(x.shape), float(t), None if y is None else y.tolist()))
        return -0.5 * x

    y = torch.randn(3, 784)
    t = torch.tensor(0.25)
    sde = SF2MSDE(model, score, sigma=0.1)
    assert sde.noise_type == "diagonal" and sde.sde_type == "ito"
    f = sde.f(t, y)
    assert f.shape == y.shape
    torch.testing.assert_close(f, (2.0 * y + 0.25) + (-0.5 * y), rtol=0, atol=0)
    assert seen == [("m", (3, 1, 28, 28), 0.25, None), ("s", (3, 1, 28, 28), 0.25, None)]
    seen.clear()
    lab = torch.tensor([1, 2, 3])
    rev = SF2MSDE(model, score, labels=lab, reverse=True, sigma=0.1)
    f = rev.f(t, y)
    assert f.shape == y.shape
    torch.testing.assert_close(f, -(2.0 * y + 0.75) + (-0.5 * y), rtol=0, atol=0)
    assert seen == [("m", (3, 1, 28, 28), 0.75, [1, 2, 3]), ("s", (3, 1, 28, 28), 0.75, [1, 2, 3])]
    g = rev.g(t, y)
    assert g.shape == y.shape and bool((g == torch.tensor(0.1, dtype=torch.float32)).all())
    # the image view follows the model's own geometry when it has one
    from torchcfm_compat import UNetModelWrapper

    m3 = UNetModelWrapper(dim=(3, 16, 16), num_channels=32, num_res_blocks=1, channel_mult=(1, 2), attention_resolutions="8")
    assert SF2MSDE(m3, m3)._image_shape() == (3, 16, 16)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

def test_restatement_against_hand_computed_linear_drifts():
    """With linear 'nets' drift = p*x + t and score = q*x the restatement's two steps match the hand-computed recursion (fp64), forward and
    reverse, and its interpolated output is the hand-computed one."""
    def lin(sd, cfg, x, t, y):
        return sd["k"] * x + (sd["c"] * t).reshape(-1, 1, 1, 1)

    dsd, ssd = {"k": 0.5, "c": 1.0}, {"k": -2.0, "c": 0.0}
    x0 = torch.tensor([[[[1.0, -2.0]]], [[[0.5, 3.0]]]])
    grid = [0.0, 0.25, 0.75]
    dW = torch.tensor([[[[[0.1, -0.3]]], [[[0.2, 0.0]]]], [[[[-0.4, 0.5]]], [[[0.05, 0.1]]]]])
    sigma = 0.2
    for reverse in (False, True):
        x = x0.double()
        xs = [x]
        for k in range(2):
            t = grid[k]
            te = 1 - t if reverse else t
            a = 0.5 * x + te
            b = -2.0 * x
            f = -a + b if reverse else a + b
            x = x + f * (grid[k + 1] - grid[k]) + sigma * dW[k].double()
            xs.append(x)
        got, outs = sf2m_euler_ref(dsd, ssd, None, x0, grid, dW, sigma, reverse=reverse, outputs=[(0, 0.0), (1, 0.5), (1, 1.0)], forward=lin)
        torch.testing.assert_close(got.double(), xs[2], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(outs[0], x0, rtol=0, atol=0)
        torch.testing.assert_close(outs[1].double(), xs[1] + 0.5 * (xs[2] - xs[1]), rtol=1e-6, atol=1e-6)
        assert torch.equal(outs[2], got)


def test_restatement_with_the_oracle_net_is_deterministic_and_uses_labels(golden):
    """One step of the real restatement on the class-conditional MNIST fixture's geometry: the label term changes the result, sigma*dW
    enters linearly."""
    from image_diffusion.unet import param_shapes
    from mi355.synth import randn, synth_state_dict
    from tests.test_classcond_cpu import load_case

    g, cfg = load_case(golden, "mnist")
    dsd = synth_state_dict(param_shapes(cfg), 11)
    ssd = synth_state_dict(param_shapes(cfg), 12)
    x0 = randn(13, 2, 1, 28, 28)
    dW = randn(14, 1, 2, 1, 28, 28) * 0.1
    grid = [0.0, 0.01]
    a, _ = sf2m_euler_ref(dsd, ssd, cfg, x0, grid, dW, 0.1)
    b, _ = sf2m_euler_ref(dsd, ssd, cfg, x0, grid, dW, 0.1)
    assert torch.equal(a, b)
    c, _ = sf2m_euler_ref(dsd, ssd, cfg, x0, grid, dW, 0.1, labels=torch.tensor([3, 7]))
    assert (a - c).abs().max() > 1e-5
    z, _ = sf2m_euler_ref(dsd, ssd, cfg, x0, grid, torch.zeros_like(dW), 0.1)
    torch.testing.assert_close(a - z, 0.1 * dW[0], rtol=0, atol=1e-6)
    assert math.isfinite(float(a.abs().max()))


# ---- the library ----------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported():
    import __graft_entry__ as ge

    ge.build()
    from mi355 import _lib

    L = _lib.lib()
    for name in ("mi355_sf2m_euler_sample", "mi355_sde_euler_step"):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
    assert L.mi355_version() == 108
