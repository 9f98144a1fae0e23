"""CPU: the adaptive Dormand-Prince solver (mi355/ode.py) against answers it does not share a source with - the order conditions of
its coefficient tables, the analytic solution of a linear system, scipy's RK45 - and the host-loop noise offsets of the samplers.

`Dopri5` runs on a torch stand-in for its three device ops (the op table is injectable); where an order is measured the state and the
stand-in are fp64, so rounding does not mask it.  No GPU, no HIP library."""
import math

import pytest
import torch

from mi355.ode import ALPHA, BETA, C_ERROR, C_MID, Dopri5


class CpuOps:
    """The three RK ops of csrc/ode.hip in eager torch, in the dtype of the tensors they are given."""

    def __init__(self):
        self.interp_calls = 0

    def rk_combine(self, out, y0, ks, coeffs):
        acc = torch.zeros_like(out)
        for k, c in zip(ks, coeffs):
            acc = acc + k * c
        out.copy_(acc if y0 is None else y0 + acc)
        return out

    def rk_sqnorm(self, acc, a, sub=None, b=None, b2=None, atol=1.0, rtol=0.0):
        num = a if sub is None else a - sub
        mag = torch.zeros_like(a) if b is None else b.abs()
        if b2 is not None:
            mag = torch.maximum(mag, b2.abs())
        r = num / (atol + rtol * mag)
        acc += (r.double() ** 2).sum()
        return acc

    def rk_interp(self, out, y0, y1, ymid, f0, f1, dt, x):
        self.interp_calls += 1
        a = 2 * dt * (f1 - f0) - 8 * (y1 + y0) + 16 * ymid
        b = dt * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * ymid
        c = dt * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * ymid
        d = dt * f0
        out.copy_((((a * x + b) * x + c) * x + d) * x + y0)
        return out


# ---- the coefficient tables ----------------------------------------------------------------------------------------------------------

def _butcher():
    A = torch.zeros(7, 7, dtype=torch.float64)
    for i, row in enumerate(BETA):
        A[i + 1, : len(row)] = torch.tensor(row, dtype=torch.float64)
    c = torch.tensor([0.0] + ALPHA, dtype=torch.float64)
    return A, c


def _order_conditions(b, A, c, theta=1.0):
    """{order: [residuals]} of the rooted-tree conditions sum_i b_i Phi_i(tree) = theta^order / gamma(tree), orders 1..5 (17 trees)."""
    Ac, Ac2, Ac3 = A @ c, A @ c ** 2, A @ c ** 3
    AAc = A @ Ac
    trees = {
        1: [(torch.ones_like(c), 1)],
        2: [(c, 2)],
        3: [(c ** 2, 3), (Ac, 6)],
        4: [(c ** 3, 4), (c * Ac, 8), (Ac2, 12), (AAc, 24)],
        5: [(c ** 4, 5), (c ** 2 * Ac, 10), (Ac * Ac, 20), (c * Ac2, 15), (Ac3, 20), (c * AAc, 30), (A @ (c * Ac), 40), (A @ Ac2, 60),
            (A @ AAc, 120)],
    }
    return {p: [abs(float(b @ phi) - theta ** p / gamma) for phi, gamma in ts] for p, ts in trees.items()}


def test_alpha_is_the_row_sum_of_beta():
    for a, row in zip(ALPHA, BETA):
        assert abs(a - math.fsum(row)) <= 1e-14, (a, row)       # measured: <= 1.2e-16


def test_solution_weights_satisfy_all_17_conditions_through_order_5():
    A, c = _butcher()
    b = torch.tensor(BETA[-1] + [0.0], dtype=torch.float64)
    res = _order_conditions(b, A, c)
    assert sum(len(v) for v in res.values()) == 17
    worst = max(max(v) for v in res.values())
    print(f"dopri5 b: worst residual through order 5 = {worst:.2e}")
    assert worst <= 1e-14                                       # measured: 9.7e-17


def test_embedded_weights_are_order_4_and_not_order_5():
    A, c = _butcher()
    bhat = torch.tensor(BETA[-1] + [0.0], dtype=torch.float64) - torch.tensor(C_ERROR, dtype=torch.float64)
    res = _order_conditions(bhat, A, c)
    low = max(max(res[p]) for p in (1, 2, 3, 4))
    print(f"dopri5 b - C_ERROR: worst residual through order 4 = {low:.2e}, worst order-5 residual = {max(res[5]):.2e}")
    assert sum(len(res[p]) for p in (1, 2, 3, 4)) == 8
    assert low <= 1e-14                                         # measured: 8.3e-17
    assert max(res[5]) > 1e-4                                   # measured: 5.4e-4 (the estimate is the order-5 term, not zero)


def test_midpoint_weights_satisfy_the_half_step_conditions_through_order_4():
    A, c = _butcher()
    res = _order_conditions(torch.tensor(C_MID, dtype=torch.float64), A, c, theta=0.5)
    low = max(max(res[p]) for p in (1, 2, 3, 4))               # 1/2, 1/8, 1/24, 1/48, 1/64, 1/128, 1/192, 1/384
    print(f"dopri5 C_MID: worst half-step residual through order 4 = {low:.2e}")
    assert low <= 1e-14                                         # measured: 2.8e-17


# ---- a linear problem with a closed-form solution ---------------------------------------------------------------------------------------

N, ROWS = 64, 8


def _problem(dtype=torch.float64):
    """y' = y S^T, S = 1.5 (W - W^T) / sqrt(n) - 0.3 I: rotation at rates up to ~3 with a slow decay; y(t) = y0 expm(t S)^T."""
    g = torch.Generator().manual_seed(20240)
    W = torch.randn(N, N, generator=g, dtype=torch.float64)
    S = 1.5 * (W - W.T) / math.sqrt(N) - 0.3 * torch.eye(N, dtype=torch.float64)
    y0 = torch.randn(ROWS, N, generator=g, dtype=torch.float64)
    St = S.T.contiguous().to(dtype)
    return S, y0, (lambda t, y: [y[0] @ St])


def _exact(S, y0, t):
    return y0 @ torch.linalg.matrix_exp(t * S).T


def _one_step(h):
    S, y0, f = _problem()
    sol = Dopri5(f, 1e-6, 1e-6, ops=CpuOps(), dtype=torch.float64)
    f0 = sol._f(0.0, [y0])
    y1, f1, err, ks = sol._step(0.0, h, [y0], f0)
    ymid = sol._midpoint([y0], ks, h)
    interp = ([y0], y1, ymid, f0, f1, 0.0, h)
    assert sol.nfe == 7
    return S, y0, sol, y1[0], ymid[0], err[0], interp


def _orders(errs):
    return [math.log2(errs[i] / errs[i + 1]) for i in range(len(errs) - 1)]


HS = (0.2, 0.1, 0.05)


def test_local_order_of_the_step_the_midpoint_and_the_error_estimate():
    e1, em, ee = [], [], []
    for h in HS:
        S, y0, _, y1, ymid, err, _ = _one_step(h)
        e1.append((y1 - _exact(S, y0, h)).abs().max().item())
        em.append((ymid - _exact(S, y0, h / 2)).abs().max().item())
        ee.append(err.abs().max().item())
    o1, om, oe = _orders(e1), _orders(em), _orders(ee)
    print(f"one step, h = {HS}: |y1 - exact| {e1} order {o1}; |ymid - exact| {em} order {om}; |err| {ee} order {oe}")
    assert min(o1) >= 5.5       # measured: 6.05, 6.01 (local error of a 5th-order step: h^6)
    assert min(om) >= 4.5       # measured: 5.37, 4.96 (4th-order midpoint: h^5)
    assert 4.5 <= min(oe) and max(oe) <= 5.6    # measured: 4.91, 4.96 (difference of a 5th- and a 4th-order state: h^5)


@pytest.mark.parametrize("x", [0.25, 0.5, 0.8])
def test_local_order_of_the_dense_output(x):
    errs = []
    for h in HS:
        S, y0, sol, _, _, _, interp = _one_step(h)
        errs.append((sol._dense(interp, x * h)[0] - _exact(S, y0, x * h)).abs().max().item())
    o = _orders(errs)
    print(f"dense output at x = {x}: errors {errs}, order {o}")
    assert min(o) >= 4.5        # measured: 5.06, 4.88 (x = 0.25); 5.37, 4.96 (0.5); 5.97, 5.39 (0.8)


def test_dense_output_passes_through_its_three_nodes():
    S, y0, sol, y1, ymid, _, interp = _one_step(0.1)
    for x, want in ((0.0, y0), (1.0, y1), (0.5, ymid)):
        got = sol._dense(interp, x * 0.1)[0]
        rel = ((got - want).abs().max() / want.abs().max()).item()
        print(f"dense output at x = {x}: relative difference to the node {rel:.2e}")
        assert rel <= 1e-12     # measured: 0 (x = 0), 5.1e-15 (x = 1), 6.3e-16 (x = 0.5)


TIMES = [0.0, 0.25, 0.6, 1.0]


def solve_cpu(tol, dtype=torch.float32):
    """The section's problem through Dopri5 on the CPU stand-in -> (solver, [state at TIMES[1:]])."""
    S, y0, f = _problem(dtype)
    sol = Dopri5(f, tol, tol, ops=CpuOps(), dtype=dtype)
    outs = sol.integrate_times([y0.to(dtype)], TIMES)
    return sol, [o[0] for o in outs]


@pytest.mark.parametrize("tol", [1e-3, 1e-4, 1e-5, 1e-6])
def test_adaptive_solve_against_the_analytic_solution(tol):
    S, y0, _ = _problem()
    sol, outs = solve_cpu(tol)
    y0r = y0.float().double()       # the solver starts from the fp32-rounded state
    ratios = [((o.double() - _exact(S, y0r, t)).abs().max().item()) / tol for o, t in zip(outs, TIMES[1:])]
    print(f"adaptive fp32, tol {tol:g}: max|err| / tol at t = {TIMES[1:]}: {ratios}, nfe {sol.nfe}, rejected {sol.n_rejected}")
    assert outs[0].dtype == torch.float32 and sol.nfe == 6 * sol.n_steps + 2
    # measured (err / tol at 0.25, 0.6, 1.0; nfe): 1e-3: 3.7, 6.1, 8.5, 26;  1e-4: 1.4, 5.5, 7.3, 38;  1e-5: 2.8, 4.7, 6.9, 50;
    # 1e-6: 2.1, 3.6, 7.4, 74.  A wrong dense-output or table entry gives O(1) errors = 1e3 .. 1e6 tol.
    assert max(ratios) <= 20.0


@pytest.mark.parametrize("tol", [1e-4, 1e-6])
def test_against_scipy_rk45(tol):
    """scipy's RK45 is the same Dormand-Prince pair written by other hands, with its own controller and dense output."""
    integrate = pytest.importorskip("scipy.integrate")
    S, y0, _ = _problem()
    y0r = y0.float().double()
    Sn = S.numpy()
    r = integrate.solve_ivp(lambda t, y: (y.reshape(ROWS, N) @ Sn.T).ravel(), (0.0, 1.0), y0r.numpy().ravel(), method="RK45", rtol=tol, atol=tol)
    assert r.success
    sol, outs = solve_cpu(tol)
    diff = (outs[-1].double() - torch.from_numpy(r.y[:, -1]).reshape(ROWS, N)).abs().max().item()
    print(f"tol {tol:g}: |ours - scipy| / tol = {diff / tol:.2f}; nfe ours {sol.nfe}, scipy {r.nfev}")
    assert diff <= 20 * tol                 # measured: 1e-4: 3.8 tol;  1e-6: 6.1 tol
    assert sol.nfe <= 1.5 * r.nfev + 12     # measured: 38 vs 38 (1e-4), 74 vs 80 (1e-6)


# ---- controller paths --------------------------------------------------------------------------------------------------------------------

def test_a_stiff_problem_rejects_steps_and_still_converges():
    """y' = -lam (y - cos t) with lam = 400: the step grows on the smooth solution until it passes the stability limit (3.3 / lam), the
    error estimate explodes and the controller has to reject."""
    lam = 400.0
    ts = []

    def f(t, y):
        ts.append(t)
        return [-lam * (y[0] - math.cos(t))]

    sol = Dopri5(f, 1e-4, 1e-4, ops=CpuOps(), dtype=torch.float64)
    y0 = torch.ones(5, dtype=torch.float64)
    out = sol.integrate([y0], 0.0, 2.0)[0]
    # the smooth solution: y = (lam^2 cos t + lam sin t) / (lam^2 + 1) + c exp(-lam t), the transient is gone at t = 2
    want = (lam * lam * math.cos(2.0) + lam * math.sin(2.0)) / (lam * lam + 1)
    print(f"stiff: steps {sol.n_steps}, rejected {sol.n_rejected}, nfe {sol.nfe}, |err| {(out - want).abs().max().item():.2e}")
    assert sol.n_rejected >= 1                      # measured: 60 rejected of 304 steps
    assert sol.n_steps * 6 + 2 == sol.nfe == len(ts)
    assert (out - want).abs().max().item() <= 20 * 1e-4     # measured: 1.0e-4


def test_step_factor_uses_the_fifth_root_of_the_error_ratio():
    """The local error of the pair is C h^5, so a step scaled by 0.9 / ratio**(1/5) lands on the ratio 0.9^5 = 0.5905 whatever the last
    one was; a smooth problem at a tight tolerance (fp64: C changes by a few per cent per step, nothing rounds) sits there step after
    step.  Any other exponent settles elsewhere (1/4: at 0.9^4 = 0.656, after an oscillation)."""

    class Recording(CpuOps):
        ratios = None

        def rk_sqnorm(self, acc, a, sub=None, b=None, b2=None, atol=1.0, rtol=0.0):
            before = acc.item()
            super().rk_sqnorm(acc, a, sub, b, b2, atol, rtol)
            if b2 is not None:      # the accept / reject ratio is the one norm scaled by max(|y0|, |y1|)
                self.ratios.append(math.sqrt((acc.item() - before) / a.numel()))
            return acc

    _, y0, f = _problem()
    ops = Recording()
    ops.ratios = []
    sol = Dopri5(f, 1e-9, 1e-9, ops=ops, dtype=torch.float64)
    sol.integrate([y0], 0.0, 1.0)
    settled = ops.ratios[3:]
    print(f"error ratios of {sol.n_steps} steps at tol 1e-9: first {ops.ratios[:4]}, then {min(settled):.4f} .. {max(settled):.4f}")
    assert sol.n_steps == len(ops.ratios) >= 30 and sol.n_rejected == 0     # measured: 45 steps, none rejected
    assert 0.9 ** 5 * 0.95 <= min(settled) and max(settled) <= 0.9 ** 5 * 1.05     # measured: 0.5814 .. 0.5938 (0.9^5 = 0.5905)


def test_output_time_equal_to_the_start_time():
    S, y0, f = _problem(torch.float32)
    ops = CpuOps()
    sol = Dopri5(f, 1e-4, 1e-4, ops=ops)
    y32 = y0.float()
    outs = sol.integrate_times([y32], [0.0, 0.0, 0.5])
    assert torch.equal(outs[0][0], y32) and outs[0][0] is not y32
    assert ops.interp_calls == 1
    assert (outs[1][0].double() - _exact(S, y32.double(), 0.5)).abs().max().item() <= 20 * 1e-4


def test_tuple_state_norm_is_the_maximum_over_components():
    sol = Dopri5(lambda t, y: y, 1e-3, 1e-3, ops=CpuOps())
    a, b = torch.full((10,), 1.0), torch.full((1000,), 3.0)
    assert sol._norm([a, b]) == pytest.approx(3.0, rel=1e-12)          # not the pooled rms sqrt((10 + 9000) / 1010) = 2.987
    assert sol._norm([b, a]) == pytest.approx(3.0, rel=1e-12)
    assert sol._norm([a * 4, b]) == pytest.approx(4.0, rel=1e-12)      # ... and not simply the last or the largest component
    # end to end: a large inert component (y = 0, y' = 0) never wins the maximum, so the solve takes exactly the steps of the active
    # component alone; a norm pooled over all elements would dilute the error 11-fold and take fewer
    S, y0, f = _problem(torch.float32)
    single = Dopri5(f, 1e-5, 1e-5, ops=CpuOps())
    want = single.integrate([y0.float()], 0.0, 1.0)[0]
    pair = Dopri5(lambda t, y: [f(t, [y[0]])[0], torch.zeros_like(y[1])], 1e-5, 1e-5, ops=CpuOps())
    got = pair.integrate([y0.float(), torch.zeros(10 * ROWS * N)], 0.0, 1.0)
    print(f"tuple state: nfe {pair.nfe} (single {single.nfe})")
    assert pair.nfe == single.nfe and torch.equal(got[0], want) and not got[1].any()    # measured: 50 and 50


def test_max_num_steps_raises():
    _, y0, f = _problem(torch.float32)
    sol = Dopri5(f, 1e-6, 1e-6, ops=CpuOps(), max_num_steps=3)
    with pytest.raises(RuntimeError, match="max_num_steps"):
        sol.integrate([y0.float()], 0.0, 1.0)
    assert sol.n_steps == 3


# ---- host-loop noise offsets ---------------------------------------------------------------------------------------------------------------

def test_host_loop_noise_offsets_never_overlap(monkeypatch):
    """Successive sampler calls on the host-loop path (one `_Noise` each) with different batch sizes: every draw owns its own
    [off, off + stride) of the seed's Philox stream, counters stay whole (off % 4 == 0) and a process's first call starts at 0."""
    from image_diffusion import sampling

    monkeypatch.setattr(sampling, "_draw_counter", 0)
    monkeypatch.setattr(sampling, "_noise_offset", 0)
    monkeypatch.setattr(sampling, "_injected", None)
    torch.manual_seed(11)
    ranges = []
    for numel, draws in ((1000, 10), (100, 10), (7, 3), (4099, 2), (1000, 1)):
        noise = sampling._Noise(torch.empty(numel))
        assert noise.stride == (numel + 3) // 4 * 4
        for k in range(draws):
            z, (seed, off) = noise.next()
            assert z is None and seed == 11 and off % 4 == 0
            if not ranges:
                assert off == 0
            if len(ranges) < 10:
                assert off == k * 1000      # a process's first call: draw k at k * stride, as mi355_ddpm_sample numbers them
            ranges.append((off, off + noise.stride))
    ranges.sort()
    for (a0, a1), (b0, b1) in zip(ranges, ranges[1:]):
        assert a1 <= b0, ((a0, a1), (b0, b1))
    assert sampling._draw_counter == 26


def test_fast_path_keys_stay_distinct_between_and_after_host_loop_calls(monkeypatch):
    from image_diffusion import sampling
    from image_diffusion.sde_diffusion import DDPM

    monkeypatch.setattr(sampling, "_draw_counter", 0)
    monkeypatch.setattr(sampling, "_noise_offset", 0)
    monkeypatch.setattr(sampling, "_injected", None)
    torch.manual_seed(11)
    seeds = []

    class Engine:
        def ddpm_sample(self, x, tables, **kw):
            seeds.append(kw["seed"])

    ddpm = DDPM(25)
    x = torch.zeros(2, 1, 4, 4)
    sampling._run_fast(Engine(), ddpm, x, 0, None)
    sampling._run_fast(Engine(), ddpm, x, 0, None)
    noise = sampling._Noise(x)
    noise.next(), noise.next()
    sampling._run_fast(Engine(), ddpm, x, 0, None)
    assert len(set(seeds)) == 3 and all(0 <= s < 1 << 63 for s in seeds)
    assert seeds[0] == (11 + 0x9E3779B97F4A7C15) & ((1 << 63) - 1)      # the first call's key is what it has always been
