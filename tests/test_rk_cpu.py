"""CPU: the fixed-step explicit Runge-Kutta samplers' host parts - the tableaus of mi355.ode.TABLEAUS against their order conditions in
exact rational arithmetic, the measured convergence order of mi355.ode.FixedStepRK on a problem with a closed-form solution, the host
plumbing (nfe, grids, tuple states, NeuralODE's solver names, refusals) and `fixed_rk_ref`, the textbook restatement of one fixed-step
solve that tests/test_gpu_rk.py holds the HIP loop (mi355_cfm_rk_sample) to.

Neither torchdyn nor torchdiffeq is vendored: which of their solver names means which table is recalled, not checked ('parity unpinned');
the tables themselves are textbook (Hairer, Norsett, Wanner I, II.1) and `REF_TABLEAUS` below is this file's own copy of them.
"""
import math
from fractions import Fraction as Fr

import pytest
import torch

# name -> (a rows below the diagonal, b, c, order): written out here, not read from the product
REF_TABLEAUS = {
    "euler": ([[]], [1], [0], 1),
    "midpoint": ([[], [Fr(1, 2)]], [0, 1], [0, Fr(1, 2)], 2),
    "heun2": ([[], [1]], [Fr(1, 2), Fr(1, 2)], [0, 1], 2),
    "rk4": ([[], [Fr(1, 2)], [0, Fr(1, 2)], [0, 0, 1]], [Fr(1, 6), Fr(1, 3), Fr(1, 3), Fr(1, 6)], [0, Fr(1, 2), Fr(1, 2), 1], 4),
    "rk4_38": ([[], [Fr(1, 3)], [Fr(-1, 3), 1], [1, -1, 1]], [Fr(1, 8), Fr(3, 8), Fr(3, 8), Fr(1, 8)], [0, Fr(1, 3), Fr(2, 3), 1], 4),
}


def ref_tableau(name):
    """REF_TABLEAUS[name] as floats: (a [s][s] zero-padded, b, c)."""
    a, b, c, _ = REF_TABLEAUS[name]
    s = len(b)
    return [[float(r[j]) if j < len(r) else 0.0 for j in range(s)] for r in a], [float(v) for v in b], [float(v) for v in c]


def fixed_rk_ref(f, x0, t_span, tableau, dtype=torch.float32):
    """One fixed-step explicit Runge-Kutta solve of x' = f(t, x), one step per interval of t_span, in eager torch of `dtype`:
    k_i = f(T_i, x + sum_{j<i} (dt a_ij) k_j), x <- x + sum_j (dt b_j) k_j with dt = t_{k+1} - t_k and T_i = t_k (c_i == 0), t_{k+1}
    (c_i == 1) or t_k + c_i dt; the sums run in index order from zero over the non-zero coefficients.  f(t, x): t a 0-dim tensor.
    tableau: (a [s][s], b, c) floats.  -> all len(t_span) states."""
    a, b, c = tableau
    s = len(b)
    x = x0.to(dtype).clone()
    traj = [x.clone()]
    sc = lambda v: torch.tensor(float(v), dtype=dtype)   # noqa: E731
    for k in range(len(t_span) - 1):
        t0, t1 = sc(t_span[k]), sc(t_span[k + 1])
        dt = t1 - t0
        ks = []
        for i in range(s):
            ti = t0 if c[i] == 0 else (t1 if c[i] == 1 else t0 + sc(c[i]) * dt)
            yi = x
            if any(a[i][j] != 0 for j in range(i)):
                acc = torch.zeros_like(x)
                for j in range(i):
                    if a[i][j] != 0:
                        acc = acc + ks[j] * (dt * sc(a[i][j]))
                yi = x + acc
            ks.append(f(ti, yi).to(dtype))
        acc = torch.zeros_like(x)
        for j in range(s):
            if b[j] != 0:
                acc = acc + ks[j] * (dt * sc(b[j]))
        x = x + acc
        traj.append(x.clone())
    return torch.stack(traj)


class CpuOps:
    """mi355_rk_stage in eager torch, in the dtype of the tensors it is given; records its calls."""

    def __init__(self):
        self.calls = []

    def rk_stage(self, out, y0, ks, coeffs, copy_out=None, u8_out=None):
        assert 1 <= len(ks) == len(coeffs) <= 4
        self.calls.append((len(ks), [float(c) for c in coeffs]))
        acc = torch.zeros_like(y0)
        for k, c in zip(ks, coeffs):
            acc = acc + k * c
        r = y0 + acc
        out.copy_(r)
        if copy_out is not None:
            copy_out.copy_(r)
        if u8_out is not None:
            u8_out.copy_((r * 127.5 + 128).clip(0, 255).to(torch.uint8))
        return out


# ---- the tables ---------------------------------------------------------------------------------------------------------------------

def _conditions(a, b, c):
    """Residuals of the rooted-tree order conditions, grouped by order 1..4, plus the bushy-tree condition of order 5."""
    s = len(b)
    A = [[Fr(a[i][j]) if j < len(a[i]) else Fr(0) for j in range(s)] for i in range(s)]
    b, c = [Fr(v) for v in b], [Fr(v) for v in c]
    R = range(s)
    Ac = [sum(A[i][j] * c[j] for j in R) for i in R]
    Ac2 = [sum(A[i][j] * c[j] ** 2 for j in R) for i in R]
    AAc = [sum(A[i][j] * Ac[j] for j in R) for i in R]
    return {
        1: [sum(b) - 1],
        2: [sum(b[i] * c[i] for i in R) - Fr(1, 2)],
        3: [sum(b[i] * c[i] ** 2 for i in R) - Fr(1, 3), sum(b[i] * Ac[i] for i in R) - Fr(1, 6)],
        4: [sum(b[i] * c[i] ** 3 for i in R) - Fr(1, 4), sum(b[i] * c[i] * Ac[i] for i in R) - Fr(1, 8),
            sum(b[i] * Ac2[i] for i in R) - Fr(1, 12), sum(b[i] * AAc[i] for i in R) - Fr(1, 24)],
        5: [sum(b[i] * c[i] ** 4 for i in R) - Fr(1, 5)],
    }


@pytest.mark.parametrize("name", sorted(REF_TABLEAUS))
def test_tableau_order_conditions(name):
    """The product's table, exactly: c_i = sum_j a_ij, strictly lower triangular, every condition up to its order (all eight through
    order 4 for the two 4-stage tables), and not the first condition of the next order."""
    from mi355.ode import TABLEAUS

    order = REF_TABLEAUS[name][3]
    a, b, c = TABLEAUS[name]
    s = len(b)
    assert len(a) == len(c) == s and all(len(r) == s for r in a)
    assert all(isinstance(v, (Fr, int)) for r in a for v in r) and all(isinstance(v, (Fr, int)) for v in list(b) + list(c))
    for i in range(s):
        assert all(a[i][j] == 0 for j in range(i, s)), "strictly lower triangular"
        assert sum(a[i]) == c[i]
    cond = _conditions(a, b, c)
    for o in range(1, order + 1):
        assert all(r == 0 for r in cond[o]), (name, o, cond[o])
    assert cond[order + 1][0] != 0, f"{name} would be of order {order + 1}"
    assert sum(len(cond[o]) for o in range(1, 5)) == 8
    # and it is the textbook table
    ra, rb, rc, _ = REF_TABLEAUS[name]
    assert [list(r[:i]) for i, r in enumerate(a)] == [[Fr(v) for v in r] + [Fr(0)] * (i - len(r)) for i, r in enumerate(ra)]
    assert list(b) == [Fr(v) for v in rb] and list(c) == [Fr(v) for v in rc]


def test_resolve_tableau():
    from mi355.ode import TABLEAUS, resolve_tableau

    assert set(TABLEAUS) == set(REF_TABLEAUS)
    for name in REF_TABLEAUS:
        assert resolve_tableau(name) == ref_tableau(name)
    a, b, c = resolve_tableau(([[], [0.5]], [0, 1], [0, 0.5]))      # short rows are padded
    assert (a, b, c) == ref_tableau("midpoint")
    with pytest.raises(NotImplementedError):
        resolve_tableau("rk5")
    with pytest.raises(ValueError):
        resolve_tableau(([[0.5], [0.5]], [0, 1], [0, 0.5]))            # an implicit entry
    with pytest.raises(ValueError):
        resolve_tableau(([[]] * 5, [0.2] * 5, [0] * 5))                # five stages
    with pytest.raises(ValueError):
        resolve_tableau(([[]], [1], [0, 1]))


def test_resolve_tableau_refuses_degenerate_triples():
    """A caller's own triple: weights that are all zero (the step would be x + 0 * k_1, which carries a NaN of k_1 into x) and stage times
    that do not belong to the stage states (c_i != sum_j a_ij) are refused; thirds written in decimals pass."""
    from mi355.ode import resolve_tableau

    with pytest.raises(ValueError, match="all zero"):
        resolve_tableau(([[], [0.5]], [0, 0], [0, 0.5]))
    with pytest.raises(ValueError, match="sum_j a_ij"):
        resolve_tableau(([[], [0.5]], [0, 1], [0, 0.75]))
    with pytest.raises(ValueError, match="sum_j a_ij"):
        resolve_tableau(([[]], [1], [0.5]))
    a, b, c = resolve_tableau(([[], [0.3333333], [-0.3333333, 1], [1, -1, 1]], [0.125, 0.375, 0.375, 0.125], [0, 0.3333333, 0.6666667, 1]))
    assert len(b) == 4 and a[2][:2] == [-0.3333333, 1.0]


# ---- convergence ----------------------------------------------------------------------------------------------------------------------

W = 2.0


def _A(t):
    ct = math.cos(float(t))
    return torch.tensor([[-ct, -W], [W, -ct]], dtype=torch.float64)


def _exact(t, y0):
    """y' = (-cos t I + W J) y: the two parts commute, y(t) = exp(-sin t) R(W t) y0."""
    cw, sw = math.cos(W * t), math.sin(W * t)
    return math.exp(-math.sin(t)) * (torch.tensor([[cw, -sw], [sw, cw]], dtype=torch.float64) @ y0)


@pytest.mark.parametrize("name", sorted(REF_TABLEAUS))
def test_measured_global_order(name):
    """FixedStepRK (fp64 op table) on the non-autonomous linear system above over [0, 2]: the global error at 16, 32, 64, 128 steps gives
    three order estimates log2(e_N / e_2N); each within 0.3 of the method's order.  A wrong coefficient that keeps the row sums (so that a
    typo-free check of the table against itself would pass) shows here."""
    from mi355.ode import FixedStepRK

    order = REF_TABLEAUS[name][3]
    y0 = torch.tensor([1.0, 0.5], dtype=torch.float64)
    errs = []
    for n in (16, 32, 64, 128):
        sol = FixedStepRK(lambda t, y: [_A(t) @ y[0]], name, ops=CpuOps(), dtype=torch.float64)
        ts = [2.0 * k / n for k in range(n + 1)]
        out = sol.integrate_times([y0], ts)[-1][0]
        assert sol.nfe == len(REF_TABLEAUS[name][1]) * n
        errs.append((out - _exact(2.0, y0)).abs().max().item())
    orders = [math.log2(errs[i] / errs[i + 1]) for i in range(3)]
    print(f"{name}: errors {['%.3e' % e for e in errs]}, measured orders {['%.3f' % o for o in orders]} (nominal {order})")
    for o in orders:
        assert abs(o - order) < 0.3, (name, orders)


# ---- host plumbing --------------------------------------------------------------------------------------------------------------------

def _field(t, y):
    return torch.stack([-y[1] * (1 + t), y[0] + torch.sin(t) * y[1]])


@pytest.mark.parametrize("grid", [[0.0, 0.05, 0.07, 0.5, 1.0], [1.0, 0.6, 0.55, 0.0], [0.3, 0.9]])
@pytest.mark.parametrize("name", ["midpoint", "heun2", "rk4", "rk4_38"])
def test_host_loop_matches_the_restatement_on_any_grid(name, grid):
    """Non-uniform and decreasing grids, fp64: FixedStepRK (rk_stage op table) against fixed_rk_ref, every state; nfe = stages * steps."""
    from mi355.ode import FixedStepRK

    y0 = torch.tensor([0.7, -0.2], dtype=torch.float64)
    ops = CpuOps()
    sol = FixedStepRK(lambda t, y: [_field(torch.tensor(t, dtype=torch.float64), y[0])], name, ops=ops, dtype=torch.float64)
    outs = sol.integrate_times([y0], grid)
    ref = fixed_rk_ref(_field, y0, grid, ref_tableau(name), dtype=torch.float64)
    stages = len(REF_TABLEAUS[name][1])
    assert sol.nfe == stages * (len(grid) - 1)
    assert len(outs) == len(grid) - 1
    for k, o in enumerate(outs):
        torch.testing.assert_close(o[0], ref[k + 1], rtol=1e-13, atol=1e-14)
    assert (ref[-1] - y0).abs().max() > 0.1
    # launches: one rk_stage per stage with a non-zero row (all but the first) and one for the update, each over its non-zero coefficients
    a, b, _ = ref_tableau(name)
    want = [sum(v != 0 for v in a[i]) for i in range(1, stages)] + [sum(v != 0 for v in b)]
    assert [n for n, _ in ops.calls] == want * (len(grid) - 1)
    if name == "rk4":
        assert want == [1, 1, 1, 4]


def test_tuple_state_and_fp32():
    """A two-component state integrates as the concatenated system does; the default dtype is fp32 with fp32 host scalars."""
    from mi355.ode import FixedStepRK

    grid = [0.0, 0.3, 0.35, 1.0]
    y0 = torch.tensor([0.7, -0.2])

    def f2(t, y):
        v = _field(torch.tensor(t), torch.stack([y[0][0], y[1][0]]))
        return [v[0:1], v[1:2]]

    sol = FixedStepRK(f2, "rk4", ops=CpuOps())
    outs = sol.integrate_times((y0[0:1], y0[1:2]), grid)
    ref = fixed_rk_ref(_field, y0, grid, ref_tableau("rk4"))
    assert sol.nfe == 4 * 3 and all(len(o) == 2 and o[0].dtype == torch.float32 for o in outs)
    for k, o in enumerate(outs):
        torch.testing.assert_close(torch.cat(o), ref[k + 1], rtol=1e-6, atol=1e-7)
    assert torch.equal(sol.integrate((y0[0:1], y0[1:2]), 0.0, 0.0)[0], y0[0:1])   # an empty interval: the state itself


def test_neural_ode_solver_names(monkeypatch):
    """NeuralODE(solver="midpoint") over a plain callable: the host loop, two rk_stage launches per step (the stage state over dt / 2, the
    update over dt alone: b_1 = 0 is skipped); all len(t_span) states come back; unknown names still raise."""
    import mi355.ode
    from torchcfm_compat import NeuralODE

    rec = CpuOps()
    monkeypatch.setattr(mi355.ode, "default_ops", rec)
    seen = []

    def vf(t, x):
        seen.append(float(t))
        return -x * (1 + t)

    x0 = torch.tensor([[1.0, 2.0, -1.0]])
    ts = torch.tensor([0.0, 0.25, 1.0])
    traj = NeuralODE(vf, solver="midpoint").trajectory(x0, ts)
    assert traj.shape == (3, 1, 3) and torch.equal(traj[0], x0)
    assert rec.calls == [(1, [0.125]), (1, [0.25]), (1, [0.375]), (1, [0.75])]
    assert seen == [0.0, 0.125, 0.25, 0.625]
    ref = fixed_rk_ref(lambda t, x: -x * (1 + t), x0, ts.tolist(), ref_tableau("midpoint"))
    torch.testing.assert_close(traj, ref, rtol=1e-6, atol=1e-7)
    for name in ("heun2", "rk4", "rk4_38"):
        out = NeuralODE(vf, solver=name).trajectory(x0, ts)
        torch.testing.assert_close(out, fixed_rk_ref(lambda t, x: -x * (1 + t), x0, ts.tolist(), ref_tableau(name)), rtol=1e-6, atol=1e-7)
    for bad in ("rk5", "tsit5", "RK4"):
        with pytest.raises(NotImplementedError):
            NeuralODE(vf, solver=bad)


def test_refusals():
    """--integration_method beyond the built names, and the drifting condition with anything but Euler (refused before any device work)."""
    import compute_fid
    from mi355.engine import UNetEngine

    with pytest.raises(NotImplementedError):
        compute_fid.make_gen_1_img(None, integration_method="rk5")
    for name in ("midpoint", "heun2", "rk4", "rk4_38"):
        assert callable(compute_fid.make_gen_1_img(None, integration_method=name, device="cpu"))
    x = torch.zeros(1, 1, 28, 28)
    with pytest.raises(NotImplementedError, match="cond_drift"):
        UNetEngine.cfm_rk(None, x, [0.0, 1.0], "rk4", cond=x, cond_drift=True)
    import inspect

    sig = list(inspect.signature(UNetEngine.cfm_rk).parameters)
    assert sig[:8] == ["self", "x", "t_span", "method", "cond", "keep_traj", "want_u8", "y"]
